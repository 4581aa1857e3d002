// The ODE loop of CFM.sample (F/model/cfm.py:160-204): f5hip_cfm_sample, _masked, _units, _grids, _span and _methods, every ODE method, driven
// by ONE plan (plan_times), ONE loop over its forwards (run_sampler) and ONE update kernel (cfg_step_kernel).  Host orchestration only: the
// kernels are elementwise.h's.  Included at the end of f5hip.hip (same translation
// unit: it drives setup_sequences, the precompute_* functions and forward_step).
#pragma once

// A fixed-grid solver as data: backbone evaluations per step, and how many of their times are the step's own rows of the time table.  RK4's
// fourth stage is evaluated at t_{i+1}, the first point of the next step (or the grid's end point).
struct OdeRule { const char* name; int forwards, points; };
static const OdeRule kOdeRules[3] = {{"euler", 1, 1}, {"midpoint", 2, 2}, {"rk4", 4, 3}};

// The time of every forward of one step over [t0, t1] (t[0 .. forwards)), in fp32 and without contraction: rounded as torch rounds
// t0 + dt / 2 (midpoint), t0 + dt * (1/3) and t0 + dt * (2/3) (rk4_alt_step_func).  The only place that computes a stage time.
static void stage_times(int method, float t0, float t1, float t[4]) {
#pragma clang fp contract(off)
    const float dt = t1 - t0;
    t[0] = t0;
    if (method == 1) t[1] = t0 + 0.5f * dt;
    if (method == 2) { t[1] = t0 + dt * (1.0f / 3.0f); t[2] = t0 + dt * (2.0f / 3.0f); t[3] = t1; }
}

// The per-call arguments every sampler entry point shares (include/f5hip.h)
struct SampleArgs {
    int32_t n_utt; const int32_t *dur, *kv_len; const float* cond_dev; const uint8_t* cond_mask; const int32_t* text; int32_t nt_max;
    const float* y0_dev; float* out_dev; void* stream;
    const uint8_t* last = nullptr;   // f5hip_cfm_sample_span: per unit, != 0 = the unit ends with this call (null: every unit does)
    bool ok() const { return n_utt > 0 && dur && cond_dev && cond_mask && text && y0_dev && out_dev; }
};

// The sequences of a call's units in layout order, and what rides with them
struct UnitLayout {
    std::vector<SeqDesc> seqs;
    std::vector<float> frame_cfg;   // the strength of every frame: its unit's (cfg_unit) or the call's; 0 without an unconditional row
    std::vector<int> frame_unit;    // layout position of every frame's unit
    std::vector<uint8_t> frame_final;   // what the final select reads per frame: cond_mask of the units that end, 0 = keep the raw state (a.last only)
    std::vector<int> seq_unit;      // ... and of every sequence's
    std::vector<int> seq_end;       // seq_end[k]: sequences of the units at layout positions 0..k
    int n_frames = 0;
};

// Validates the units and lays them out in the order `order` (layout position -> unit): per unit its conditional sequence and, unless its
// strength (cfg_unit[u], or the call's) is below 1e-5, its unconditional one behind it.  Frames keep the caller's packed order.
static int layout_units(f5hip_dit* m, const SampleArgs& a, const std::vector<int>& order, float cfg_strength, const float* cfg_unit, UnitLayout& L) {
    const int n = a.n_utt;
    std::vector<int> fo(n + 1, 0);   // first frame of every unit in the caller's packed arrays
    for (int u = 0; u < n; u++) {
        if (a.dur[u] <= 0 || a.dur[u] > 4096) return fail(-1, "dur[%d] = %d out of range", u, a.dur[u]);
        const int kv = a.kv_len ? a.kv_len[u] : a.dur[u];
        if (kv <= 0 || kv > a.dur[u]) return fail(-1, "kv_len[%d] = %d out of range (1..%d)", u, kv, a.dur[u]);
        fo[u + 1] = fo[u] + a.dur[u];
    }
    L.n_frames = fo[n];
    L.frame_unit.resize(fo[n]);
    L.frame_cfg.resize(fo[n]);
    if (a.last) L.frame_final.resize(fo[n]);
    L.seq_end.resize(n);
    m->h_seq_len.clear();
    for (int k = 0; k < n; k++) {
        const int u = order[k], kv = a.kv_len ? a.kv_len[u] : a.dur[u];
        // MMDiT text stream: with batch-1 semantics a unit's text tensor is its own tokens (the reference's per-item call pads nothing); with
        // the padded-batch semantics every item carries the batch's nt positions, fillers included
        int c_len = a.nt_max;
        if (!a.kv_len) { c_len = 0; while (c_len < a.nt_max && a.text[(size_t)u * a.nt_max + c_len] != -1) c_len++; }
        // the reference's early-out (cfm.py:162-175): below 1e-5 the unconditional branch is not evaluated at all -- per call, or per unit
        const float cfg_u = cfg_unit ? cfg_unit[u] : cfg_strength;
        const bool use_cfg = !(cfg_u < 1e-5f);
        for (int f = fo[u]; f < fo[u + 1]; f++) {
            L.frame_unit[f] = k;
            L.frame_cfg[f] = use_cfg ? cfg_u : 0.0f;
            if (a.last) L.frame_final[f] = a.last[u] && a.cond_mask[f];
        }
        for (int b = 0; b < (use_cfg ? 2 : 1); b++) {
            L.seqs.push_back({a.dur[u], kv, fo[u], u, b, b, b});
            L.seqs.back().c_len = std::max(c_len, 1);
            L.seq_unit.push_back(k);
            m->h_seq_len.push_back(a.dur[u]);
        }
        L.seq_end[k] = (int)L.seqs.size();
    }
    return 0;
}

// The plan of a call: its distinct time points (the rows of the time table), and per forward f one row of (time point, CfgOp, step size) at
// [f * cols + k].  One grid and one method for all units: cols = 1, the points of the steps in sequence, `points` per step (+ the end point
// for RK4), so forward s of step i reads point i * points + s.  Otherwise cols = n, column k for the unit at layout position k, stepped by
// its own rule over its own grid: the points are the union of every unit's stage times, equal fp32 values once, and once a unit's forwards
// are done its op is CFG_OP_NONE (tp 0).  dt is the step's size, or half of it for the midpoint rule's half step.
struct TimePlan {
    int forwards = 0, cols = 1;
    std::vector<float> pts, dt;
    std::vector<int> tp, op;
};

// The forwards unit u of a call takes
static int unit_forwards(const int32_t* steps, const int32_t* method, int u) { return steps[u] * kOdeRules[method[u]].forwards; }

// order: layout position -> unit, by forwards descending.  steps / method [n] per unit; t_grid: the units' grids one after the other, or
// (per_unit false) the one grid of `steps[0]` steps they share.  Pure host code: every refusal of a grid comes before the first launch.
static int plan_times(const std::vector<int>& order, const int32_t* steps, const int32_t* method, const float* t_grid, bool per_unit, TimePlan& P) {
    static const int kFirstOp[3] = {CFG_OP_EULER, CFG_OP_MID_HALF, CFG_OP_RK4_1};
    const int n = (int)order.size();
    bool mixed = false;
    for (int u = 0; u < n; u++) mixed = mixed || method[u] != method[0];
    if (!per_unit) {
        const OdeRule& rule = kOdeRules[method[0]];
        const int end_pt = rule.forwards > rule.points ? 1 : 0;
        if ((long long)steps[0] * rule.points + end_pt > kMaxGridPoints) {
            if (method[0] == 0) return fail(-8, "at most %d time points per call (got %d)", kMaxGridPoints, steps[0]);
            return fail(-8, "%s: at most %d steps per call (got %d)", rule.name, (kMaxGridPoints - end_pt) / rule.points, steps[0]);
        }
    }
    std::map<uint32_t, int> pt_index;
    auto point = [&](float v) {
        uint32_t bits;
        memcpy(&bits, &v, sizeof(bits));
        auto it = pt_index.find(bits);
        if (it != pt_index.end()) return it->second;
        pt_index[bits] = (int)P.pts.size();
        P.pts.push_back(v);
        return (int)P.pts.size() - 1;
    };
    P.cols = per_unit ? n : 1;
    P.forwards = unit_forwards(steps, method, order[0]);
    const size_t cells = (size_t)P.forwards * P.cols;
    P.tp.assign(cells, 0);
    P.op.assign(cells, CFG_OP_NONE);
    P.dt.assign(cells, 0.0f);
    std::vector<size_t> grid0(n, 0);   // first point of every unit's grid in t_grid
    for (int u = 1; per_unit && u < n; u++) grid0[u] = grid0[u - 1] + (size_t)steps[u - 1] + 1;
    float t[4];
    for (int k = 0; k < P.cols; k++) {
        const int u = order[k], mu = method[u];
        const OdeRule& rule = kOdeRules[mu];
        const float* tg = t_grid + grid0[u];
        for (int i = 0; i < steps[u]; i++) {
            const float dt = tg[i + 1] - tg[i];
            stage_times(mu, tg[i], tg[i + 1], t);
            for (int s = 0; s < rule.forwards; s++) {
                const size_t at = ((size_t)i * rule.forwards + s) * P.cols + k;
                if (per_unit) P.tp[at] = point(t[s]);
                else {   // (RK4's fourth forward reads the next step's first point, or the end point)
                    if (s < rule.points) P.pts.push_back(t[s]);
                    P.tp[at] = i * rule.points + s;
                }
                P.op[at] = kFirstOp[mu] + s;
                P.dt[at] = mu == 1 && s == 0 ? 0.5f * dt : dt;
            }
        }
        if (!per_unit && rule.forwards > rule.points) P.pts.push_back(tg[steps[u]]);
    }
    if ((int)P.pts.size() > kMaxTimePoints)
        return fail(-8, "%s: the units' grids need %d distinct time points, at most %d per call", mixed ? "cfm_sample_methods" : "cfm_sample_grids",
                    (int)P.pts.size(), kMaxTimePoints);
    return 0;
}

// The device tables of a call with per-unit columns (in m->grid_meta), in ints: row_unit [R] | frame_unit [U] | tp | op | dt (floats)
// [forwards][n] each -- uploaded -- then row_tp [R].  The upload, the device pointers and the capacity all read the offsets here.
struct GridLayout {
    size_t row_unit, frame_unit, tp, op, dt, row_tp, total = 0;
    GridLayout(size_t R, size_t U, size_t cells) {
        auto take = [&](size_t n) { const size_t at = total; total += n; return at; };
        row_unit = take(R); frame_unit = take(U); tp = take(cells); op = take(cells); dt = take(cells); row_tp = take(R);
    }
};
struct GridTables { const int *row_unit = nullptr, *frame_unit = nullptr, *tp = nullptr, *op = nullptr; const float* dt = nullptr; int* row_tp = nullptr; };

static int upload_grid_tables(f5hip_dit* m, const UnitLayout& L, const TimePlan& P, hipStream_t st, GridTables& T) {
    const int R = m->Rtot, S = (int)L.seqs.size();
    const GridLayout g(R, L.n_frames, P.tp.size());
    if (g.total > m->grid_cap) {
        dev_free(m->grid_meta);
        m->grid_cap = 0;
        if (hipMalloc((void**)&m->grid_meta, sizeof(int) * g.total) != hipSuccess) { m->grid_meta = nullptr; return fail(-5, "hipMalloc grid tables"); }
        m->grid_cap = g.total;
    }
    std::vector<int> hb(g.row_tp, 0);
    for (int s = 0; s < S; s++) {
        for (int r = m->h_seq_row0[s]; r < m->h_seq_row0[s + 1]; r++) hb[g.row_unit + r] = L.seq_unit[s];
        for (int r = m->h_seqc_row0[s]; r < m->h_seqc_row0[s + 1]; r++) hb[g.row_unit + r] = L.seq_unit[s];
    }
    memcpy(&hb[g.frame_unit], L.frame_unit.data(), sizeof(int) * L.frame_unit.size());
    memcpy(&hb[g.tp], P.tp.data(), sizeof(int) * P.tp.size());
    memcpy(&hb[g.op], P.op.data(), sizeof(int) * P.op.size());
    memcpy(&hb[g.dt], P.dt.data(), sizeof(float) * P.dt.size());
    CK(m->up_grid.upload(m->grid_meta, hb.data(), sizeof(int) * hb.size(), st));
    int* const d = m->grid_meta;
    T = {d + g.row_unit, d + g.frame_unit, d + g.tp, d + g.op, reinterpret_cast<const float*>(d + g.dt), d + g.row_tp};
    return 0;
}

// The buffers the CFG / ODE update works on: the handle's (cfg_bufs), or a unit op's own (unit_ops.h)
struct CfgBufs {
    float *xstate, *k1, *k2, *k3;   // [U][mel]: the state; RK4's stage slopes, k1 the midpoint rule's half-step state as well (the handle's xmid)
    const float* pred;              // [rows][128]
    const int *urow_c, *urow_u;     // [U]: the frame's conditional / unconditional row (-1: none)
    const float* frame_cfg;         // [U] strengths per frame
    Plane2 xs;                      // [rows][128]: the split-bf16 copy of x the input projection reads
    int mel;
};
static CfgBufs cfg_bufs(const f5hip_dit* m) {
    return {m->xstate, m->xmid, m->rk_k2, m->rk_k3, m->pred, m->d_urow_c, m->d_urow_u, m->d_frame_cfg, m->xs, m->cfg.mel_dim};
}

// The CFG combine and ODE update of f0 frames after one forward, one launch of cfg_step_kernel.  frame_unit null: the op `op` (CfgOp) and
// step size `dt` for every frame; else per unit in layout order, unit_op / unit_dt [n] read through frame_unit, the frames of units >= n_act
// left as they are.
static void launch_cfg_step(const CfgBufs& b, int f0, int op, float dt, const int* frame_unit, const int* unit_op, const float* unit_dt, int n_act,
                            hipStream_t st) {
    auto* kernel = frame_unit ? cfg_step_kernel<true> : cfg_step_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(f0), dim3(128), 0, st, b.xstate, b.mel, f0, b.pred, 128, b.urow_c, b.urow_u, b.frame_cfg, op, dt, b.k1, b.k2, b.k3,
                       b.xs.hi, b.xs.lo, 128, frame_unit, unit_op, unit_dt, n_act);
}

// Restores the handle's full layout and per-call modulation after a sampler call, however it ends (a call with per-unit columns shrinks them)
struct GridScope {
    f5hip_dit* m;
    ~GridScope() { m->d_row_tp = nullptr; m->M = m->row_c0; m->Mc = m->Rtot - m->row_c0; m->n_seq = (int)m->h_seq_row0.size() - 1; }
};

// Every sampler call: ONE loop over the forwards of its plan (TimePlan), one launch of cfg_step_kernel after each.  steps / method [n]: the
// step count and solver of every unit.  cfg_unit null: one strength for the call (cfg_strength).
// per_unit false: the units share the grid t_grid and the solver; forward f reads row tp[f] of the time tables and every frame takes the
// same op and step size (kernel arguments; no unit tables are uploaded).
// per_unit true: unit u takes steps[u] steps by rule method[u] over its own grid, the grids one after the other in t_grid.  The units are
// laid out by their forwards, descending (stable; a unit's conditional and unconditional sequences adjacent), so the units still running at
// forward f are a prefix of the layout: the forward runs over the audio rows [0, M_f) (and MMDiT's text rows [row_c0, row_c0 + Mc_f)) of
// those units only, and the update leaves the frames of the finished units alone.  Every unit's time points go through one
// precompute_time over their union; before each forward row_tp_kernel gives every row the time point of its unit, and the modulation
// consumers read their vectors per row (m->d_row_tp; forward_step with ti = 0).
// a.last (f5hip_cfm_sample_span): the grids are spans of longer ones and y0 is the state so far; the loop is the same, and the final
// select keeps the raw state of every frame of a unit that does not end here (the per-frame flags of the metadata upload: layout_units).
static int run_sampler(f5hip_dit* m, const SampleArgs& a, const int32_t* steps, const int32_t* method, const float* t_grid, bool per_unit,
                       float cfg_strength, const float* cfg_unit) {
    const int n = a.n_utt;
    std::vector<int> order(n);
    for (int u = 0; u < n; u++) order[u] = u;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return unit_forwards(steps, method, x) > unit_forwards(steps, method, y); });
    ProfScope prof_scope(m->prof);
    hipStream_t st = (hipStream_t)a.stream;
    UnitLayout L;
    TimePlan P;
    CK(layout_units(m, a, order, cfg_strength, cfg_unit, L));
    CK(plan_times(order, steps, method, t_grid, per_unit, P));
    const int mel = m->cfg.mel_dim, U = L.n_frames;
    CK(setup_sequences(m, L.seqs, U, a.text, a.nt_max, a.cond_mask, st, L.frame_cfg.data(), a.last ? L.frame_final.data() : nullptr));
    GridScope scope{m};
    GridTables T;
    if (per_unit) CK(upload_grid_tables(m, L, P, st, T));

    if (hipMemcpyAsync(m->xstate, a.y0_dev, sizeof(float) * (size_t)U * mel, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(-6, "y0 copy");
    hipLaunchKernelGGL(split_rows_kernel, dim3(m->M), dim3(256), 0, st, m->xstate, mel, mel, m->M, m->d_row_frame, m->xs.hi, m->xs.lo, 128, 0);
    CKL("split x");
    CK(precompute_text_and_ce(m, a.cond_dev, st));
    CK(precompute_time(m, P.pts.data(), (int)P.pts.size(), st, /*reuse=*/a.last == nullptr));

    m->d_row_tp = T.row_tp;
    int n_act = n;
    for (int f = 0; f < P.forwards; f++) {
        const size_t at = (size_t)f * P.cols;
        if (per_unit) {
            while (P.op[at + n_act - 1] == CFG_OP_NONE) n_act--;   // units whose forwards are done leave the layout's tail
            const int s_act = L.seq_end[n_act - 1];
            m->M = m->h_seq_row0[s_act]; m->Mc = m->h_seqc_row0[s_act] - m->row_c0; m->n_seq = s_act;
            prof_begin(PROF_OTHER, st);
            hipLaunchKernelGGL(row_tp_kernel, dim3((m->Rtot + 255) / 256), dim3(256), 0, st, T.row_unit, T.tp + at, m->Rtot, T.row_tp);
            prof_end(PROF_OTHER, st);
            CKL("row_tp");
        }
        CK(forward_step(m, per_unit ? 0 : P.tp[at], -1, st));
        prof_begin(PROF_OTHER, st);
        launch_cfg_step(cfg_bufs(m), U, P.op[at], P.dt[at], T.frame_unit, per_unit ? T.op + at : nullptr, per_unit ? T.dt + at : nullptr, n_act, st);
        prof_end(PROF_OTHER, st);
        CKL("cfg step");
    }
    hipLaunchKernelGGL(final_select_kernel, dim3(U), dim3(128), 0, st, m->xstate, a.cond_dev, m->d_frame_is_cond, mel, U, a.out_dev);
    CKL("final_select");
    return 0;
}

// The calls whose units share one grid and one solver
static int sample_one_grid(f5hip_dit* m, const SampleArgs& a, int method, const float* t_grid, int32_t steps, float cfg_strength, const float* cfg_unit) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (!a.ok() || !t_grid || steps <= 0) return fail(-1, "cfm_sample: bad argument");
    const std::vector<int32_t> unit_steps(a.n_utt, steps), unit_method(a.n_utt, method);
    return run_sampler(m, a, unit_steps.data(), unit_method.data(), t_grid, false, cfg_strength, cfg_unit);
}

int f5hip_cfm_sample(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const float* cond_dev, const uint8_t* cond_mask,
                     const int32_t* text, int32_t nt_max, const float* y0_dev, const float* t_grid, int32_t steps,
                     float cfg_strength, float* out_dev, void* stream) {
    return sample_one_grid(m, {n_utt, dur, nullptr, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream}, m ? m->ode_method : 0, t_grid, steps, cfg_strength, nullptr);
}

int f5hip_cfm_sample_masked(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                            const int32_t* text, int32_t nt_max, const float* y0_dev, const float* t_grid, int32_t steps,
                            float cfg_strength, float* out_dev, void* stream) {
    return sample_one_grid(m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream}, m ? m->ode_method : 0, t_grid, steps, cfg_strength, nullptr);
}

int f5hip_cfm_sample_units(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                           const int32_t* text, int32_t nt_max, const float* y0_dev, const float* t_grid, int32_t steps,
                           const float* cfg_strength, float* out_dev, void* stream) {
    if (!cfg_strength) return fail(-1, "cfm_sample_units: cfg_strength is null");
    return sample_one_grid(m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream}, m ? m->ode_method : 0, t_grid, steps, 0.0f, cfg_strength);
}

// The calls with one grid per unit.  unit_method null: every unit steps by the handle's solver; else by its own (f5hip_cfm_sample_methods).
// One grid and one solver for all is f5hip_cfm_sample_units' call, kernels and results; anything else the plan with a column per unit.
static int sample_grids(const char* name, f5hip_dit* m, const SampleArgs& a, const int32_t* steps, const float* t_grids, const float* cfg_strength,
                        const int32_t* unit_method) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (!a.ok() || !steps || !t_grids || !cfg_strength) return fail(-1, "%s: bad argument", name);
    const std::vector<int32_t> handle_method(a.n_utt, m->ode_method);
    const int32_t* method = unit_method ? unit_method : handle_method.data();
    bool one = true;
    size_t g0 = 0;
    for (int u = 0; u < a.n_utt; u++) {
        if (method[u] < 0 || method[u] > 2) return fail(-1, "%s: method[%d] = %d (0 euler, 1 midpoint, 2 rk4)", name, u, method[u]);
        one = one && method[u] == method[0];
    }
    for (int u = 0; u < a.n_utt; u++) {
        if (steps[u] < 1) return fail(-1, "%s: steps[%d] = %d (need >= 1)", name, u, steps[u]);
        one = one && steps[u] == steps[0] && !memcmp(t_grids + g0, t_grids, sizeof(float) * ((size_t)steps[0] + 1));
        g0 += (size_t)steps[u] + 1;
    }
    if (one) return sample_one_grid(m, a, method[0], t_grids, steps[0], 0.0f, cfg_strength);
    return run_sampler(m, a, steps, method, t_grids, true, 0.0f, cfg_strength);
}

int f5hip_cfm_sample_grids(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                           const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                           const float* cfg_strength, float* out_dev, void* stream) {
    return sample_grids("cfm_sample_grids", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream}, steps, t_grids, cfg_strength, nullptr);
}

int f5hip_cfm_sample_span(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                          const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                          const float* cfg_strength, const uint8_t* last, float* out_dev, void* stream) {
    if (!last) return fail(-1, "cfm_sample_span: last is null");
    return sample_grids("cfm_sample_span", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream, last}, steps, t_grids, cfg_strength, nullptr);
}

int f5hip_cfm_sample_methods(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                             const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                             const float* cfg_strength, const int32_t* method, const uint8_t* last, float* out_dev, void* stream) {
    if (!method) return fail(-1, "cfm_sample_methods: method is null");
    return sample_grids("cfm_sample_methods", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream, last}, steps, t_grids,
                        cfg_strength, method);
}

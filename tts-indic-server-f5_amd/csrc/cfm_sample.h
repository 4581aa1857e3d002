// The ODE loop of CFM.sample (F/model/cfm.py:160-204): f5hip_cfm_sample, _masked, _units, _grids, _span and _methods, every ODE method, driven
// by ONE step loop (run_sampler).  Host orchestration only: the kernels are elementwise.h's.  Included at the end of f5hip.hip (same translation
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
    std::vector<float> frame_cfg;   // per-unit strengths spread over the unit's frames (cfg_unit only)
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
    if (cfg_unit) L.frame_cfg.resize(fo[n]);
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
            if (cfg_unit) L.frame_cfg[f] = use_cfg ? cfg_u : 0.0f;
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

// The time points of a call and which of them every forward evaluates.
//   One grid: the points of the steps in sequence, `points` per step (+ the end point for RK4); forward s of step i reads point
//   i * points + s of the table.
//   Mixed grids (unit_steps): the union of the units' points, equal fp32 values once; utp[f][k] = point of forward f for the unit at layout
//   position k (0 once its steps are done); udt[i][k] = dt_i and udt[max_steps + i][k] = dt_i / 2 of that unit.
//   Mixed methods (unit_method as well): the union over every unit's stage times by its own rule; per forward f and layout position k the
//   point utp[f][k], the op code uop[f][k] (CfgOp; CFG_OP_NONE once the unit's forwards are done) and the step size udt[f][k] (dt, or dt / 2
//   for the midpoint rule's half step) of cfg_mixed_kernel.  max_forwards = the forwards of the call.
struct TimePlan {
    int max_steps = 0, max_forwards = 0;
    std::vector<float> pts, udt;
    std::vector<int> utp, uop;
};

// The forwards unit u of a mixed-method call takes
static int unit_forwards(const int32_t* unit_steps, const int32_t* unit_method, int u) { return unit_steps[u] * kOdeRules[unit_method[u]].forwards; }

static int plan_times(int method, const std::vector<int>& order, const float* t_grid, int steps, const int32_t* unit_steps, const int32_t* unit_method,
                      TimePlan& P) {
    const OdeRule& rule = kOdeRules[method];
    float t[4];
    if (!unit_steps) {
        const int end_pt = rule.forwards > rule.points ? 1 : 0, n_pts = steps * rule.points + end_pt;
        if (n_pts > kMaxGridPoints) {
            if (method == 0) return fail(-8, "at most %d time points per call (got %d)", kMaxGridPoints, steps);
            return fail(-8, "%s: at most %d steps per call (got %d)", rule.name, (kMaxGridPoints - end_pt) / rule.points, steps);
        }
        P.max_steps = steps;
        for (int i = 0; i < steps; i++) {
            stage_times(method, t_grid[i], t_grid[i + 1], t);
            P.pts.insert(P.pts.end(), t, t + rule.points);
        }
        if (end_pt) P.pts.push_back(t_grid[steps]);
        return 0;
    }
    const int n = (int)order.size(), per = rule.forwards;
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
    size_t g0 = 0;
    std::vector<size_t> grid0(n);   // first point of every unit's grid in t_grid
    for (int u = 0; u < n; u++) { grid0[u] = g0; g0 += (size_t)unit_steps[u] + 1; }
    if (unit_method) {
        static const int kFirstOp[3] = {CFG_OP_EULER, CFG_OP_MID_HALF, CFG_OP_RK4_1};
        P.max_forwards = unit_forwards(unit_steps, unit_method, order[0]);
        P.utp.assign((size_t)P.max_forwards * n, 0);
        P.uop.assign((size_t)P.max_forwards * n, CFG_OP_NONE);
        P.udt.assign((size_t)P.max_forwards * n, 0.0f);
        for (int k = 0; k < n; k++) {
            const int u = order[k], mu = unit_method[u], fw = kOdeRules[mu].forwards;
            const float* tg = t_grid + grid0[u];
            for (int i = 0; i < unit_steps[u]; i++) {
                const float dt = tg[i + 1] - tg[i];
                stage_times(mu, tg[i], tg[i + 1], t);
                for (int s = 0; s < fw; s++) {
                    const size_t at = ((size_t)i * fw + s) * n + k;
                    P.utp[at] = point(t[s]);
                    P.uop[at] = kFirstOp[mu] + s;
                    P.udt[at] = mu == 1 && s == 0 ? 0.5f * dt : dt;
                }
            }
        }
        if ((int)P.pts.size() > kMaxTimePoints)
            return fail(-8, "cfm_sample_methods: the units' grids need %d distinct time points, at most %d per call", (int)P.pts.size(), kMaxTimePoints);
        return 0;
    }
    P.max_steps = unit_steps[order[0]];
    P.utp.assign((size_t)P.max_steps * per * n, 0);
    P.udt.assign((size_t)2 * P.max_steps * n, 0.0f);
    for (int k = 0; k < n; k++) {
        const float* tg = t_grid + grid0[order[k]];
        for (int i = 0; i < unit_steps[order[k]]; i++) {
            const float dt = tg[i + 1] - tg[i];
            P.udt[(size_t)i * n + k] = dt;
            P.udt[(size_t)(P.max_steps + i) * n + k] = 0.5f * dt;
            stage_times(method, tg[i], tg[i + 1], t);
            for (int s = 0; s < per; s++) P.utp[((size_t)i * per + s) * n + k] = point(t[s]);
        }
    }
    if ((int)P.pts.size() > kMaxTimePoints)
        return fail(-8, "cfm_sample_grids: the units' grids need %d distinct time points, at most %d per call", (int)P.pts.size(), kMaxTimePoints);
    return 0;
}

// The device tables of a mixed-grid call (in m->grid_meta): row_unit [R] | frame_unit [U] | utp | uop (mixed methods only) | udt (floats)
// -- uploaded -- then row_tp [R]
struct GridTables { const int *row_unit, *frame_unit, *utp, *uop; const float* udt; int* row_tp; };

static int upload_grid_tables(f5hip_dit* m, const UnitLayout& L, const TimePlan& P, hipStream_t st, GridTables& T) {
    const int R = m->Rtot, U = L.n_frames, S = (int)L.seqs.size();
    const size_t n_up = (size_t)R + U + P.utp.size() + P.uop.size() + P.udt.size(), need = n_up + R;
    if (need > m->grid_cap) {
        dev_free(m->grid_meta);
        m->grid_cap = 0;
        if (hipMalloc((void**)&m->grid_meta, sizeof(int) * need) != hipSuccess) { m->grid_meta = nullptr; return fail(-5, "hipMalloc grid tables"); }
        m->grid_cap = need;
    }
    std::vector<int> hb(n_up, 0);
    for (int s = 0; s < S; s++) {
        for (int r = m->h_seq_row0[s]; r < m->h_seq_row0[s + 1]; r++) hb[r] = L.seq_unit[s];
        for (int r = m->h_seqc_row0[s]; r < m->h_seqc_row0[s + 1]; r++) hb[r] = L.seq_unit[s];
    }
    memcpy(&hb[R], L.frame_unit.data(), sizeof(int) * U);
    memcpy(&hb[(size_t)R + U], P.utp.data(), sizeof(int) * P.utp.size());
    if (!P.uop.empty()) memcpy(&hb[(size_t)R + U + P.utp.size()], P.uop.data(), sizeof(int) * P.uop.size());
    memcpy(&hb[(size_t)R + U + P.utp.size() + P.uop.size()], P.udt.data(), sizeof(float) * P.udt.size());
    CK(m->up_grid.upload(m->grid_meta, hb.data(), sizeof(int) * n_up, st));
    T.row_unit = m->grid_meta;
    T.frame_unit = T.row_unit + R;
    T.utp = T.frame_unit + U;
    T.uop = T.utp + P.utp.size();
    T.udt = reinterpret_cast<const float*>(T.uop + P.uop.size());
    T.row_tp = m->grid_meta + n_up;
    return 0;
}

// The step of one CFG stage: one strength and step size for the call (frame_unit null; the strength per frame when the layout carries
// m->d_frame_cfg), or step sizes per unit in layout order (unit_dt; the frames of units >= n_act are left as they are).
struct CfgStep { float cfg, dt; const int* frame_unit; const float* unit_dt; int n_act; };

// The buffers one CFG stage works on: the handle's (cfg_bufs), or a unit op's own (f5hip_op_cfg_step)
struct CfgBufs {
    float *xstate, *k1, *k2, *k3;   // [U][mel]: the state (the Euler kernels' xbase), RK4's stage slopes
    const float* pred;              // [rows][128]
    const int *urow_c, *urow_u;     // [U]: the frame's conditional / unconditional row (-1: none)
    const float* frame_cfg;         // [U] strengths per frame, or null: the scalar of CfgStep
    Plane2 xs;                      // [rows][128]: the split-bf16 copy of x the input projection reads
    int mel;
};
static CfgBufs cfg_bufs(const f5hip_dit* m) {
    return {m->xstate, m->xmid, m->rk_k2, m->rk_k3, m->pred, m->d_urow_c, m->d_urow_u, m->d_frame_cfg, m->xs, m->cfg.mel_dim};
}

template <bool FRAME_CFG, bool UNIT_DT>
static void launch_cfg(const CfgBufs& b, int f0, bool rk4, int stage, float* xout, const CfgStep& c, hipStream_t st) {
    const float cfg = FRAME_CFG ? 0.0f : c.cfg, dt = UNIT_DT ? 0.0f : c.dt;
    if (rk4)
        hipLaunchKernelGGL((cfg_rk4_stage_kernel<FRAME_CFG, UNIT_DT>), dim3(f0), dim3(128), 0, st, b.xstate, b.mel, f0, b.pred, 128, b.urow_c, b.urow_u,
                           cfg, b.frame_cfg, dt, stage + 1, b.k1, b.k2, b.k3, b.xs.hi, b.xs.lo, 128, c.frame_unit, c.unit_dt, c.n_act);
    else
        hipLaunchKernelGGL((cfg_euler_kernel<FRAME_CFG, UNIT_DT>), dim3(f0), dim3(128), 0, st, xout, (const float*)b.xstate, b.mel, f0, b.pred, 128,
                           b.urow_c, b.urow_u, cfg, b.frame_cfg, dt, b.xs.hi, b.xs.lo, 128, c.frame_unit, c.unit_dt, c.n_act);
}

// One kernel instance per form of the step: <false> scalar strength, <true> per-frame strength, <true, true> per-unit dt.  rk4: stage
// `stage` + 1 of 4 in place on b.xstate; else xout = b.xstate + dt v.
static void launch_cfg_form(const CfgBufs& b, int f0, bool rk4, int stage, float* xout, const CfgStep& c, hipStream_t st) {
    if (c.frame_unit) launch_cfg<true, true>(b, f0, rk4, stage, xout, c, st);
    else if (b.frame_cfg) launch_cfg<true, false>(b, f0, rk4, stage, xout, c, st);
    else launch_cfg<false, false>(b, f0, rk4, stage, xout, c, st);
}

// The CFG combine and ODE update after forward `stage` of a step: Euler x += dt v; midpoint's first stage the half step from xstate into
// xmid (the caller passes dt / 2), its second the full step; RK4 stage `stage` + 1 of 4.
static int cfg_stage(f5hip_dit* m, int method, int stage, int f0, const CfgStep& c, hipStream_t st) {
    float* xout = method == 1 && stage == 0 ? m->xmid : m->xstate;
    prof_begin(PROF_OTHER, st);
    launch_cfg_form(cfg_bufs(m), f0, method == 2, stage, xout, c, st);
    prof_end(PROF_OTHER, st);
    CKL("cfg stage");
    return 0;
}

// The CFG combine and ODE update after one forward of a mixed-method call: every frame by its unit's op code and step size for this forward
static void launch_cfg_mixed(const CfgBufs& b, int f0, const int* frame_unit, const int* unit_op, const float* unit_dt, int n_act, hipStream_t st) {
    hipLaunchKernelGGL(cfg_mixed_kernel, dim3(f0), dim3(128), 0, st, b.xstate, b.mel, f0, b.pred, 128, b.urow_c, b.urow_u, b.frame_cfg, b.k1, b.k2, b.k3,
                       b.xs.hi, b.xs.lo, 128, frame_unit, unit_op, unit_dt, n_act);
}

// Restores the handle's full layout and per-call modulation after a sampler call, however it ends (a mixed-grid call shrinks them)
struct GridScope {
    f5hip_dit* m;
    ~GridScope() { m->d_row_tp = nullptr; m->M = m->row_c0; m->Mc = m->Rtot - m->row_c0; m->n_seq = (int)m->h_seq_row0.size() - 1; }
};

// Every sampler call.  cfg_unit null: one strength for the call (cfg_strength).  unit_steps null: the units share the grid t_grid of
// `steps` steps; else unit u takes unit_steps[u] steps over its own grid, the grids one after the other in t_grid:
// units are laid out by step count, descending (stable; a unit's conditional and unconditional sequences adjacent), so the units still
// stepping at iteration i are a prefix of the layout: the forwards of iteration i run over the audio rows [0, M_i) (and MMDiT's text rows
// [row_c0, row_c0 + Mc_i)) of those units only, and the CFG kernels leave the frames of the finished units alone.  Every unit's time points
// go through one precompute_time over their union; before each forward row_tp_kernel gives every row the time point of its unit, and the
// modulation consumers read their vectors per row (m->d_row_tp; forward_step with ti = 0).
// a.last (f5hip_cfm_sample_span): the grids are spans of longer ones and y0 is the state so far; the step loop is the same, and the final
// select keeps the raw state of every frame of a unit that does not end here (the per-frame flags of the metadata upload: layout_units).
// `method`: the solver of the call.  unit_method (f5hip_cfm_sample_methods; with unit_steps and cfg_unit, `method` unused): unit u steps by
// rule unit_method[u], F_u = unit_steps[u] * forwards of its rule.  The units are laid out by F_u, descending (stable), so those still
// running at forward f are a prefix of the layout; the loop runs over the forwards, f = 0 .. max F_u - 1: shrink to the active prefix,
// row_tp_kernel, one forward, ONE cfg_mixed_kernel launch that steps every frame by its unit's op code for this forward (TimePlan).
static int run_sampler(f5hip_dit* m, const SampleArgs& a, int method, const float* t_grid, int steps, const int32_t* unit_steps, float cfg_strength,
                       const float* cfg_unit, const int32_t* unit_method = nullptr) {
    const int n = a.n_utt, per = kOdeRules[method].forwards;
    std::vector<int> order(n);
    for (int u = 0; u < n; u++) order[u] = u;
    if (unit_method)
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return unit_forwards(unit_steps, unit_method, x) > unit_forwards(unit_steps, unit_method, y); });
    else if (unit_steps) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return unit_steps[x] > unit_steps[y]; });
    ProfScope prof_scope(m->prof);
    hipStream_t st = (hipStream_t)a.stream;
    UnitLayout L;
    TimePlan P;
    CK(layout_units(m, a, order, cfg_strength, cfg_unit, L));
    CK(plan_times(method, order, t_grid, steps, unit_steps, unit_method, P));   // (every refusal of a grid comes before the first launch)
    const int mel = m->cfg.mel_dim, U = L.n_frames;
    CK(setup_sequences(m, L.seqs, U, a.text, a.nt_max, a.cond_mask, st, cfg_unit ? L.frame_cfg.data() : nullptr, a.last ? L.frame_final.data() : nullptr));
    GridScope scope{m};
    GridTables T{};
    if (unit_steps) CK(upload_grid_tables(m, L, P, st, T));

    if (hipMemcpyAsync(m->xstate, a.y0_dev, sizeof(float) * (size_t)U * mel, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(-6, "y0 copy");
    hipLaunchKernelGGL(split_rows_kernel, dim3(m->M), dim3(256), 0, st, m->xstate, mel, mel, m->M, m->d_row_frame, m->xs.hi, m->xs.lo, 128, 0);
    CKL("split x");
    CK(precompute_text_and_ce(m, a.cond_dev, st));
    CK(precompute_time(m, P.pts.data(), (int)P.pts.size(), st));

    m->d_row_tp = T.row_tp;
    int n_act = n;
    for (int f = 0; f < P.max_forwards; f++) {   // mixed methods (max_steps is 0: the loop over the steps below does not run)
        while (unit_forwards(unit_steps, unit_method, order[n_act - 1]) <= f) n_act--;
        const int s_act = L.seq_end[n_act - 1];
        m->M = m->h_seq_row0[s_act]; m->Mc = m->h_seqc_row0[s_act] - m->row_c0; m->n_seq = s_act;
        prof_begin(PROF_OTHER, st);
        hipLaunchKernelGGL(row_tp_kernel, dim3((m->Rtot + 255) / 256), dim3(256), 0, st, T.row_unit, T.utp + (size_t)f * n, m->Rtot, T.row_tp);
        prof_end(PROF_OTHER, st);
        CKL("row_tp");
        CK(forward_step(m, 0, -1, st));
        prof_begin(PROF_OTHER, st);
        launch_cfg_mixed(cfg_bufs(m), U, T.frame_unit, T.uop + (size_t)f * n, T.udt + (size_t)f * n, n_act, st);
        prof_end(PROF_OTHER, st);
        CKL("cfg mixed");
    }
    for (int i = 0; i < P.max_steps; i++) {
        CfgStep full{cfg_strength, 0.0f, nullptr, nullptr, 0}, half = full;
        if (unit_steps) {
            while (unit_steps[order[n_act - 1]] <= i) n_act--;   // units whose steps are done leave the layout's tail
            const int s_act = L.seq_end[n_act - 1];
            m->M = m->h_seq_row0[s_act]; m->Mc = m->h_seqc_row0[s_act] - m->row_c0; m->n_seq = s_act;
            full = {0.0f, 0.0f, T.frame_unit, T.udt + (size_t)i * n, n_act};
            half = {0.0f, 0.0f, T.frame_unit, T.udt + (size_t)(P.max_steps + i) * n, n_act};
        } else {
            full.dt = t_grid[i + 1] - t_grid[i];
            half.dt = 0.5f * full.dt;
        }
        for (int s = 0; s < per; s++) {
            if (unit_steps) {
                prof_begin(PROF_OTHER, st);
                hipLaunchKernelGGL(row_tp_kernel, dim3((m->Rtot + 255) / 256), dim3(256), 0, st, T.row_unit, T.utp + ((size_t)i * per + s) * n, m->Rtot, T.row_tp);
                prof_end(PROF_OTHER, st);
                CKL("row_tp");
            }
            CK(forward_step(m, unit_steps ? 0 : i * kOdeRules[method].points + s, -1, st));
            CK(cfg_stage(m, method, s, U, method == 1 && s == 0 ? half : full, st));
        }
    }
    hipLaunchKernelGGL(final_select_kernel, dim3(U), dim3(128), 0, st, m->xstate, a.cond_dev, m->d_frame_is_cond, mel, U, a.out_dev);
    CKL("final_select");
    return 0;
}

// The calls whose units share one grid
static int sample_one_grid(f5hip_dit* m, const SampleArgs& a, int method, const float* t_grid, int32_t steps, float cfg_strength, const float* cfg_unit) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (!a.ok() || !t_grid || steps <= 0) return fail(-1, "cfm_sample: bad argument");
    return run_sampler(m, a, method, t_grid, steps, nullptr, cfg_strength, cfg_unit);
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

// The calls with one grid per unit: one grid for all is f5hip_cfm_sample_units' call, kernels and results.  unit_method null: every unit steps
// by the handle's solver; else by its own (f5hip_cfm_sample_methods) -- all equal is the call with that solver, the mixed loop otherwise.
static int sample_grids(const char* name, f5hip_dit* m, const SampleArgs& a, const int32_t* steps, const float* t_grids, const float* cfg_strength,
                        const int32_t* unit_method = nullptr) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (!a.ok() || !steps || !t_grids || !cfg_strength) return fail(-1, "%s: bad argument", name);
    int method = m->ode_method;
    if (unit_method) {
        bool one_method = true;
        for (int u = 0; u < a.n_utt; u++) {
            if (unit_method[u] < 0 || unit_method[u] > 2) return fail(-1, "%s: method[%d] = %d (0 euler, 1 midpoint, 2 rk4)", name, u, unit_method[u]);
            one_method = one_method && unit_method[u] == unit_method[0];
        }
        if (one_method) { method = unit_method[0]; unit_method = nullptr; }
    }
    bool one_grid = true;
    size_t g0 = 0;
    for (int u = 0; u < a.n_utt; u++) {
        if (steps[u] < 1) return fail(-1, "%s: steps[%d] = %d (need >= 1)", name, u, steps[u]);
        one_grid = one_grid && steps[u] == steps[0] && !memcmp(t_grids + g0, t_grids, sizeof(float) * ((size_t)steps[0] + 1));
        g0 += (size_t)steps[u] + 1;
    }
    if (unit_method) return run_sampler(m, a, 0, t_grids, 0, steps, 0.0f, cfg_strength, unit_method);
    if (one_grid) return sample_one_grid(m, a, method, t_grids, steps[0], 0.0f, cfg_strength);
    return run_sampler(m, a, method, t_grids, 0, steps, 0.0f, cfg_strength);
}

int f5hip_cfm_sample_grids(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                           const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                           const float* cfg_strength, float* out_dev, void* stream) {
    return sample_grids("cfm_sample_grids", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream}, steps, t_grids, cfg_strength);
}

int f5hip_cfm_sample_span(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                          const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                          const float* cfg_strength, const uint8_t* last, float* out_dev, void* stream) {
    if (!last) return fail(-1, "cfm_sample_span: last is null");
    return sample_grids("cfm_sample_span", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream, last}, steps, t_grids, cfg_strength);
}

int f5hip_cfm_sample_methods(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev, const uint8_t* cond_mask,
                             const int32_t* text, int32_t nt_max, const float* y0_dev, const int32_t* steps, const float* t_grids,
                             const float* cfg_strength, const int32_t* method, const uint8_t* last, float* out_dev, void* stream) {
    if (!method) return fail(-1, "cfm_sample_methods: method is null");
    return sample_grids("cfm_sample_methods", m, {n_utt, dur, kv_len, cond_dev, cond_mask, text, nt_max, y0_dev, out_dev, stream, last}, steps, t_grids,
                        cfg_strength, method);
}

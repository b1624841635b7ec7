// libjmid_hip.so -- the C ABI proper (include/jmid_hip.h): handle lifetime, the compute entry points, knobs, streams.
#include "jmid_ctx.hpp"
#include "collision_stats.hpp"
#include "wall_stats.hpp"
#include "repair.hpp"

namespace jmid_host {

// The wall segments of a call: a HOST array [L, 4] fp64 in both memory modes.  Checked here (finite, 0 <= L <= 64) and sent ahead of the
// kernels through the handle's own staging; *dev: where they lie on the device (null with L = 0)
int upload_walls(jmid_ctx* h, int L, const double* walls, const double** dev, const std::string& who) {
    *dev = nullptr;
    if (L < 0 || L > WLS_MAX_L) return fail(h, JMID_EINVAL, who + " supports 0 <= L <= 64 walls");
    if (L == 0) return 0;
    if (!walls) return fail(h, JMID_EINVAL, who + ": null walls with L > 0");
    for (int i = 0; i < L * 4; ++i)
        if (!std::isfinite(walls[i])) return fail(h, JMID_EINVAL, who + ": a wall has a non-finite coordinate");
    if (int rc = h->wall_seg.upload(h, walls, L * 8, who.c_str())) return rc;
    *dev = h->wall_seg.get<double>();
    return 0;
}

std::string& thread_error() {
    static thread_local std::string e;
    return e;
}

int fail(jmid_ctx* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    thread_error() = msg;
    return code;
}

// pos = NULL of jmid_topk / jmid_eval_statistics: the positions the most recent jmid_denoise left in the workspace, or null (with the
// error set) when there are none of this shape - the rules include/jmid_hip.h documents at jmid_topk
const float* resident_positions(jmid_ctx* h, int E, int A, int K, int T) {
    if (!h->last_pos || h->last_pos_dims[0] != E || h->last_pos_dims[1] != A || h->last_pos_dims[2] != K || h->last_pos_dims[3] != T) {
        fail(h, JMID_EINVAL, "pos = NULL needs a preceding jmid_denoise with p0 and the same E, A, K, T on this handle");
        return nullptr;
    }
    return h->last_pos;
}

// The KDE's workspace, laid out here only: ll [E, T, K] doubles | Y, the whitened points [E, T, K, 2 A], only when they do not fit in
// LDS (E = 64, T = 12, K = 1024, A = 32 would be 400 MB).  base null: the size only
size_t kde_workspace(int E, int A, int K, int T, char* base, KdeArgs* g) {
    Carver c(base);
    double* ll = c.take<double>((size_t)E * T * K);
    double* Y = c.take<double>(kde_y_in_lds(A, K) ? 0 : (size_t)E * T * K * 2 * A);
    if (g) g->ll = ll, g->Y = Y;
    return c.off;
}

// the two KDE launches on device buffers (pos [E, K, A, T, 2], bw [T] or null -> sel, logw).  ws: kde_workspace bytes the caller staged,
// or null: the handle's second workspace
int topk_on_device(jmid_ctx* h, const char* who, int E, int A, int K, int T, int k, const float* pos, const float* bw, float* sel, float* logw,
                   const int* n_agents_dev, char* ws = nullptr) {
    if (!ws) {
        if (int rc = h->kde_ws.reserve(h, kde_workspace(E, A, K, T, nullptr, nullptr), who)) return rc;
        ws = h->kde_ws.p;
    }
    KdeArgs g{};
    g.E = E; g.A = A; g.K = K; g.T = T; g.k = k;
    kde_workspace(E, A, K, T, ws, &g);
    g.pos = pos; g.bw = bw; g.sel = sel; g.logw = logw; g.n_agents = n_agents_dev;
    ProfScope ps(h, KC_TOPK, h->stream);
    HIPCHK(h, launch_kde(g, h->stream));
    return 0;
}

// the encoder's launch arguments: the handle's transposed LSTM / attention weights, the caller's n rows
EncArgs encoder_args(const jmid_ctx* h, const float* x_st, const float* nbr_sum, const float* edge_mask, float* ctx, int n) {
    EncArgs ea{};
    ea.x_st = x_st; ea.nbr_sum = nbr_sum; ea.edge_mask = edge_mask;
    ea.hist = LstmW{h->lstmT[0][0], h->lstmT[0][1], h->lstmT[0][2]};
    ea.edge[0] = LstmW{h->lstmT[1][0], h->lstmT[1][1], h->lstmT[1][2]};
    ea.edge[1] = LstmW{h->lstmT[2][0], h->lstmT[2][1], h->lstmT[2][2]};
    ea.W1T = h->attW1T; ea.W2T = h->attW2T; ea.v = h->wt.edge_v;
    ea.ctx = ctx; ea.n = n; ea.Th = h->hist_len; ea.H = h->H;
    return ea;
}

// The I/O block of a chained call, laid out here only: the upload block (x_st, nbr_sum, edge_mask, x_T, p0, bw: contiguous, one copy; in
// scene mode the copy starts at x_T and the gather overwrites the p0 slot after it, on the stream) | ctx | the download block (flag,
// forecasts, their logw, sel, logw, pos: contiguous, one copy, ending behind the assembled arrays of a forecast) | the dense [E * A] copy of
// a resident scene's first_index.  pinned: the handle's pinned block instead - upload + download and nothing else, with the same inner
// offsets.  A constrained chain (c.cons) adds its four report arrays behind the forecasts' logw, inside the download block of either form,
// and - with repair, on the device only - the predicates' lean values at the very end; without constraints both layouts are what they
// always were.  base null: the size only
size_t chain_io(const jmid_ctx* h, const ChainCall& c, char* base, ChainIo* out, bool pinned) {
    const size_t n = (size_t)c.E * c.A, Th = h->hist_len, n_xT = (size_t)c.E * c.K * c.A * c.T * 2, Np = c.forecast ? h->scene.N : 0;
    Carver cv(base);
    ChainIo io{};
    io.x_st = cv.arr(n * Th * 6); io.nbr_sum = cv.arr(n * 2 * Th * 6); io.edge_mask = cv.arr(n * 2);
    io.x_T = cv.arr(n_xT); io.p0 = cv.arr(n * 2); io.bw = cv.arr(c.rank() && c.bw ? c.T : 0);
    io.up_bytes = cv.off;
    if (!pinned) io.ctx = cv.arr(n * 2 * h->H);
    const size_t down = cv.off;
    io.flag = cv.arr<int>(1); io.forecasts = cv.arr<double>((size_t)c.E * Np * c.k * (c.T + 1) * 2); io.logw_d = cv.arr<double>((size_t)c.E * Np * c.k);
    if (c.cons) {      // a constrained chain: the four reports, inside the download block of either form (nothing of this without constraints)
        const size_t EK = (size_t)c.E * c.K;
        io.guide = cv.arr(EK * GDE_COLS); io.rsample = cv.arr(EK * RPR_SAMPLE_COLS); io.repisode = cv.arr<int>((size_t)c.E * RPR_EPISODE_COLS);
        io.rwall = cv.arr(EK * RPR_WALL_COLS);
    }
    if (c.forecast) io.down_bytes = cv.off - down;
    if (!c.forecast || !pinned) io.sel = cv.arr(c.rank() ? n * c.k * c.T * 2 : 0), io.logw = cv.arr(c.rank() ? n * c.k : 0), io.pos = cv.arr(c.pos_out ? n_xT : 0);
    if (!c.forecast) io.down_bytes = cv.off - down;
    if (!pinned && c.scene && h->scene.has_first()) io.first_index = cv.arr<int>(n);
    if (!pinned && c.cons && c.cons->repair) io.gate = cv.arr<double>((size_t)c.E * c.K * (CLS_WS_COLS + WLS_WS_COLS));
    if (out) *out = io;
    return cv.off;
}

// What the phases of one chained call share: its device and pinned blocks as chain_io laid them out, and the device counts of a padded
// scene chain (the n_in the build kernel wrote), null otherwise
struct ChainRun {
    ChainIo dev, pin;
    const int* nag_dev = nullptr;
    const double* walls = nullptr;      // a constrained chain with walls: where upload_walls put them, once, for the guidance and the repair
};

int reserve_chain_io(jmid_ctx* h, const ChainCall& c, Block& b, bool pinned, ChainIo* io) {
    if (int rc = b.reserve(h, chain_io(h, c, nullptr, nullptr, pinned), c.who)) return rc;
    chain_io(h, c, b.p, io, pinned);
    return 0;
}

// phase 1: the host inputs through the pinned block in one copy; a seeded x_T is filled in its slot on the device
int stage_inputs(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const ChainIo &dev = r.dev, &pin = r.pin;
    if (!c.seeded) std::memcpy(pin.x_T.p, c.x_T, pin.x_T.bytes());
    if (pin.bw.n) std::memcpy(pin.bw.p, c.bw, pin.bw.bytes());
    if (!c.scene) {
        std::memcpy(pin.x_st.p, c.x_st, pin.x_st.bytes()); std::memcpy(pin.nbr_sum.p, c.nbr_sum, pin.nbr_sum.bytes());
        std::memcpy(pin.edge_mask.p, c.edge_mask, pin.edge_mask.bytes()); std::memcpy(pin.p0.p, c.p0, pin.p0.bytes());
        HIPCHK(h, hipMemcpyAsync(dev.x_st.p, pin.x_st.p, dev.up_bytes, hipMemcpyHostToDevice, h->stream));
    } else if (!c.seeded) {
        // x_T ... bw in one copy (the p0 slot between them is written by the gather, after the copy on the stream)
        HIPCHK(h, hipMemcpyAsync(dev.x_T.p, pin.x_T.p, dev.up_bytes_from(dev.x_T), hipMemcpyHostToDevice, h->stream));
    } else if (dev.bw.n) {
        HIPCHK(h, hipMemcpyAsync(dev.bw.p, pin.bw.p, dev.bw.bytes(), hipMemcpyHostToDevice, h->stream));
    }
    if (c.seeded) {
        if (int rc = h->noise_ids.upload(h, c.seeded->ids, c.E, c.who)) return rc;
        if (r.nag_dev) return fill_noise_padded(h, c.seeded->seed, h->noise_ids.get<unsigned>(), r.nag_dev, c.E, c.A, c.K, c.T, 0, dev.x_T, h->stream);
        return fill_noise(h, c.seeded->seed, h->noise_ids.get<unsigned>(), c.E, (size_t)c.K * c.A * c.T * 2, 0, dev.x_T, nullptr, h->stream);
    }
    return 0;
}

// phase 2: (scene: the in-cluster rows of the resident scene into the upload block's slots, then) the encoder -> ctx
int gather_encode(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const ChainIo& dev = r.dev;
    ProfScope ps(h, KC_ENCODER, h->stream);
    if (c.scene) {
        const SceneArrays& sa = h->scene.arr;
        SceneGatherArgs ga{};
        ga.in_cluster = sa.in_cluster;
        ga.x_st = sa.x_st; ga.nbr_sum = sa.nbr_sum; ga.edge_mask = sa.edge_mask; ga.p0 = sa.p0;
        ga.o_x_st = dev.x_st; ga.o_nbr_sum = dev.nbr_sum; ga.o_edge_mask = dev.edge_mask; ga.o_p0 = dev.p0;
        ga.first_index = sa.first_index; ga.o_first_index = dev.first_index;      // (both null for a scene without one)
        ga.E = c.E; ga.N = h->scene.N; ga.A = c.A; ga.F = h->hist_len; ga.pad = r.nag_dev ? 1 : 0;
        if (launch_scene_gather(ga, h->stream) != hipSuccess) return fail(h, JMID_EHIP, std::string(c.who) + ": scene gather launch failed");
    }
    EncArgs ea = encoder_args(h, dev.x_st, dev.nbr_sum, dev.edge_mask, dev.ctx, c.E * c.A);
    ea.first_index = dev.first_index;
    if (launch_encoder(ea, h->stream) != hipSuccess) return fail(h, JMID_EHIP, std::string(c.who) + ": encoder launch failed");
    return 0;
}

// phase 3: the denoise loop and the integrator as a stage of the chain - no caller-stream ordering, the flag comes with the one download
int denoise_stage(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    DenoiseCall d{c.E, c.A, c.K, c.T, c.precision, JMID_MEM_DEVICE};
    d.x_in = r.dev.x_T; d.ctx = r.dev.ctx; d.p0 = r.dev.p0; d.dt = c.dt; d.pos_out = r.dev.pos; d.chained = true;
    d.n_agents = c.n_agents; d.n_agents_dev = r.nag_dev; d.who = c.who;
    GuideCall gc;
    if (const ChainConstraints* k = c.cons) {
        if (k->repair) d.pos_out = nullptr;      // (the repair phase copies the set out once it has repaired it)
        if (k->guided()) {      // the guide kernel reads the chain's own p0 slot and the counts the denoise call has anyway
            gc.threshold = k->threshold; gc.margin = k->guide_margin; gc.tau = k->guide_tau; gc.weights = k->guide_weights; gc.n_inner = k->n_inner;
            gc.L = k->guide_walls ? k->L : 0; gc.walls = gc.L ? r.walls : nullptr; gc.wall_radius = k->guide_walls ? k->wall_radius : 0.0;
            gc.guide_out = r.dev.guide;
            d.guide = &gc;
        }
    }
    return run_network(h, d);
}

// phase 3b (a constrained chain with repair): the launches of jmid_repair_collisions[_walls](pos = NULL) on the set the denoise stage left,
// in place, on the handle's stream - the ranking and the assembly then read the repaired set, and with pos_out the block is copied out
// here.  (A variant of the repair kernel that evaluates the candidate gate itself, one launch instead of three or four, was measured
// inside this phase and did not pay: docs/NOTEBOOK.md section 41)
int repair_samples(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const ChainConstraints& k = *c.cons;
    const int E = c.E, A = c.A, K = c.K, T = c.T, L = k.repair_walls ? k.L : 0;
    const int* nag = r.nag_dev ? r.nag_dev : c.padded ? h->nag.get<int>() : nullptr;      // (host arrays: the denoise stage's upload)
    const size_t lean = (size_t)E * K * CLS_WS_COLS;
    CollisionStatsArgs cs{};
    cs.E = E; cs.A = A; cs.K = K; cs.T = T; cs.threshold = k.threshold;
    cs.pos = h->last_pos; cs.ws = r.dev.gate.p; cs.n_agents = nag;
    WallStatsArgs ws{};
    ws.E = E; ws.A = A; ws.K = K; ws.T = T; ws.L = L; ws.radius = k.wall_radius;
    ws.walls = L > 0 ? r.walls : nullptr; ws.pos = h->last_pos; ws.n_agents = nag;
    ws.p0 = L > 0 ? r.dev.p0.p : nullptr;      // (the first point of every path; without walls the repair reads no p0)
    ws.ws = L > 0 ? r.dev.gate.p + lean : nullptr;
    RepairWallArgs g{};
    g.E = E; g.A = A; g.K = K; g.T = T; g.max_iter = k.max_iter;
    g.threshold = k.threshold; g.margin = k.margin; g.tau = k.tau; g.step = k.step; g.dt = (double)c.dt;
    g.L = L; g.walls = ws.walls; g.wall_radius = k.repair_walls ? k.wall_radius : 0.0;
    g.src = h->last_pos; g.dst = const_cast<float*>(h->last_pos); g.p0 = ws.p0; g.n_agents = nag;
    g.sample = r.dev.rsample; g.episode = r.dev.repisode; g.wall_out = r.dev.rwall;
    g.ws = cs.ws; g.wws = ws.ws;
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_collision_stats(cs, h->stream));
        if (L > 0) HIPCHK(h, launch_wall_stats(ws, h->stream));
        HIPCHK(h, launch_repair_walls(g, h->stream));      // (L = 0: jmid_repair_collisions' launches, +inf in the wall rows)
    }
    if (r.dev.pos.n) HIPCHK(h, hipMemcpyAsync(r.dev.pos.p, h->last_pos, r.dev.pos.bytes(), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// phase 4 (k < K): the KDE ranks the positions the denoise stage left in the workspace -> sel, logw
int rank_samples(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const int* nag = r.nag_dev ? r.nag_dev : c.padded ? h->nag.get<int>() : nullptr;      // (host arrays: the denoise stage's upload)
    return topk_on_device(h, c.who, c.E, c.A, c.K, c.T, c.k, h->last_pos, r.dev.bw, r.dev.sel, r.dev.logw, nag);
}

// phase 5 (forecast): assemble_kernel -> forecasts [E, N, k, T+1, 2] and logw [E, N, k] doubles over every pedestrian of the scene
int assemble_forecasts(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const jmid_ctx::SceneWs& sc = h->scene;
    const size_t Th = h->hist_len;
    AssembleArgs aa{};
    aa.in_cluster = sc.arr.in_cluster;
    aa.src = c.rank() ? r.dev.sel.p : h->last_pos;
    aa.logw_in = r.dev.logw;
    aa.cv = sc.arr.cv;
    // pose_now: its own slot after a stamped build, the last frame of the grid otherwise (what predict_batch prepends)
    aa.pose = sc.stamped ? sc.arr.grid.pose_now.p : sc.arr.grid.human_xy.p + (Th - 1) * (size_t)sc.N * 2;
    aa.pose_stride = sc.stamped ? (size_t)sc.N * 2 : Th * (size_t)sc.N * 2;
    aa.forecasts = r.dev.forecasts;
    aa.logw = r.dev.logw_d;
    aa.logw_full = std::log(1.0 / (double)c.K);
    aa.E = c.E; aa.N = sc.N; aa.A = c.A; aa.k = c.k; aa.T = c.T; aa.full = c.rank() ? 0 : 1;
    aa.first_index = sc.arr.first_index;                      // (null for a scene without one) -1: the track's rows are NaN
    if (launch_assemble(aa, h->stream) != hipSuccess) return fail(h, JMID_EHIP, std::string(c.who) + ": assemble launch failed");
    return 0;
}

// phase 6: the range flag joins the download block, one copy, the one synchronisation, the caller's arrays
int finish_chain(jmid_ctx* h, const ChainCall& c, const ChainRun& r) {
    const ChainIo &dev = r.dev, &pin = r.pin;
    const bool flagged = c.precision != JMID_PREC_F32;
    if (flagged) HIPCHK(h, hipMemcpyAsync(dev.flag.p, h->range_flag, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(pin.flag.p, dev.flag.p, dev.down_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flagged && *pin.flag.p) return jmid_host::flagged_call(h, *pin.flag.p);
    if (const ChainConstraints* k = c.cons) {      // the reports came with the same copy
        if (k->guide_out) std::memcpy(k->guide_out, pin.guide.p, pin.guide.bytes());
        if (k->sample_out) std::memcpy(k->sample_out, pin.rsample.p, pin.rsample.bytes());
        if (k->episode_out) std::memcpy(k->episode_out, pin.repisode.p, pin.repisode.bytes());
        if (k->wall_out) std::memcpy(k->wall_out, pin.rwall.p, pin.rwall.bytes());
    }
    if (c.forecast) {
        std::memcpy(c.forecasts_out, pin.forecasts.p, pin.forecasts.bytes());
        std::memcpy(c.logw_out, pin.logw_d.p, pin.logw_d.bytes());
        return JMID_OK;
    }
    if (c.rank()) {
        std::memcpy(c.sel, pin.sel.p, pin.sel.bytes());
        std::memcpy(c.logw, pin.logw.p, pin.logw.bytes());
    }
    if (c.pos_out) std::memcpy(c.pos_out, pin.pos.p, pin.pos.bytes());
    return JMID_OK;
}

// A chained call after its entry's argument checks (every refusal has come by then: nothing is enqueued for a call that is refused)
int predict_chain(jmid_ctx* h, const ChainCall& c) {
    ChainRun r;
    if (c.scene && c.padded) r.nag_dev = h->scene.arr.n_in;
    if (int rc = reserve_chain_io(h, c, h->io_dev, false, &r.dev)) return rc;
    if (int rc = reserve_chain_io(h, c, h->pin, true, &r.pin)) return rc;
    if (const ChainConstraints* k = c.cons) {
        // the walls go up once and serve both mechanisms; the report rows of a mechanism that is off are zero (state 0, no guided step)
        if (k->walled())
            if (int rc = upload_walls(h, k->L, k->walls, &r.walls, c.who)) return rc;
        char* const z0 = (char*)(k->guided() ? r.dev.rsample.p : r.dev.guide.p);
        char* const z1 = k->repair ? (char*)r.dev.rsample.p : (char*)r.dev.rwall.p + align_up(r.dev.rwall.bytes());
        if (z1 > z0) HIPCHK(h, hipMemsetAsync(z0, 0, (size_t)(z1 - z0), h->stream));
    }
    int rc = stage_inputs(h, c, r);
    if (!rc) rc = gather_encode(h, c, r);
    if (!rc) rc = denoise_stage(h, c, r);
    if (!rc && c.cons && c.cons->repair) rc = repair_samples(h, c, r);
    if (!rc && c.rank()) rc = rank_samples(h, c, r);
    if (!rc && c.forecast) rc = assemble_forecasts(h, c, r);
    return rc ? rc : finish_chain(h, c, r);
}

// where the grid of a scene lies in a workspace: human_xy [E, F, N, 2] | robot_xy [E, F, 2] | pose_now [E, N, 2] doubles.  base null: the size only
size_t grid_block(int E, int N, int F, char* base, GridBlock* out) {
    Carver c(base);
    GridBlock gb{};
    gb.human_xy = c.arr<double>((size_t)E * F * N * 2); gb.robot_xy = c.arr<double>((size_t)E * F * 2);
    gb.xy_bytes = c.off;
    gb.pose_now = c.arr<double>((size_t)E * N * 2);
    if (out) *out = gb;
    return c.off;
}

// The scene workspace, laid out here only (horizon 0: no cv), the grid block its prefix.  base null: the size only
size_t scene_arrays(int E, int N, int F, int horizon, bool has_first, char* base, SceneArrays* out) {
    const size_t rows = (size_t)E * N;
    SceneArrays a{};
    Carver c(base);
    c.off = grid_block(E, N, F, base, &a.grid);
    a.x = c.arr(rows * F * 6); a.x_st = c.arr(rows * F * 6); a.nbr_sum = c.arr(rows * 2 * F * 6); a.edge_mask = c.arr(rows * 2); a.p0 = c.arr(rows * 2);
    const size_t down = c.off;
    a.n_in = c.arr<int>(E); a.in_cluster = c.arr<unsigned char>(rows); a.robot_in = c.arr<unsigned char>(E); a.cv = c.arr<double>(rows * horizon * 2);
    a.down_bytes = c.off - down;
    if (has_first) a.first_index = c.arr<int>(rows);
    if (out) *out = a;
    return c.off;
}

// the refusals jmid_build_scene and jmid_build_scene_stamped share (F is the handle's hist_len by then)
int check_scene_dims(jmid_ctx* h, const char* who, int N, int F, const double* cv_out, int horizon, double time_step) {
    const std::string w(who);
    if (F != h->hist_len || F < 3 || F > SCN_MAX_F) return fail(h, JMID_EINVAL, w + ": F must be the handle's hist_len, and at least 3");
    if (N < 1 || N > SCN_LANES - 1) return fail(h, JMID_EINVAL, w + " supports 1 <= N <= 63 pedestrians");
    if (cv_out && (horizon < 1 || horizon > SCN_MAX_H)) return fail(h, JMID_EINVAL, w + ": the horizon of cv_out must be in 1..24");
    if (!(time_step > 0.0) || !std::isfinite(time_step)) return fail(h, JMID_EINVAL, w + ": time_step must be finite and > 0");
    return 0;
}

// A scene build after its entry's argument checks and order_in: the grid into the scene workspace, scene_kernel, the small outputs to the
// caller (`mem` says where they live), one synchronisation
int build_scene_resident(jmid_ctx* h, const SceneBuild& b) {
    const bool host = b.mem == JMID_MEM_HOST;
    const int E = b.E, N = b.N, F = b.F, horizon = b.cv_out ? b.horizon : 0;
    jmid_ctx::SceneWs& sc = h->scene;
    sc.E = 0;                     // no scene is resident until this call has succeeded
    if (int rc = sc.dev.reserve(h, scene_arrays(E, N, F, horizon, b.first_frame != nullptr, nullptr, nullptr), b.who)) return rc;
    SceneArrays a;
    scene_arrays(E, N, F, horizon, b.first_frame != nullptr, sc.dev.p, &a);
    SceneArgs g{};
    g.E = E; g.N = N; g.F = F; g.horizon = b.horizon; g.force_all = b.force_all_in_cluster ? 1 : 0;
    g.dt = b.time_step;
    g.human_xy = a.grid.human_xy; g.robot_xy = a.grid.robot_xy;
    g.x = a.x; g.x_st = a.x_st; g.nbr_sum = a.nbr_sum; g.edge_mask = a.edge_mask; g.p0 = a.p0;
    g.n_in = a.n_in; g.in_cluster = a.in_cluster; g.robot_in = a.robot_in; g.cv = a.cv;
    if (b.first_frame) {
        if (int rc = h->first_idx.upload(h, b.first_frame, E * (N + 1), b.who)) return rc;
        g.first_frame = h->first_idx.get<int>();
        g.first_index = a.first_index;
    }
    // the pinned block: human_xy | robot_xy of a host build, as the grid block has them | the download block (device mode: n_in alone)
    const size_t pin_in = b.src == SCENE_HOST_ARRAYS ? a.grid.xy_bytes : 0, b_nin = a.n_in.bytes();
    if (int rc = h->pin.reserve(h, pin_in + (host ? a.down_bytes : b_nin), b.who)) return rc;
    char* const pin = h->pin.p;
    if (b.src == SCENE_HOST_ARRAYS) {
        GridBlock pg;
        grid_block(E, N, F, pin, &pg);
        std::memcpy(pg.human_xy.p, b.human_xy, pg.human_xy.bytes()); std::memcpy(pg.robot_xy.p, b.robot_xy, pg.robot_xy.bytes());
        HIPCHK(h, hipMemcpyAsync(sc.dev.p, pin, pin_in, hipMemcpyHostToDevice, h->stream));
    } else if (b.src == SCENE_DEVICE_ARRAYS) {
        HIPCHK(h, hipMemcpyAsync(a.grid.human_xy.p, b.human_xy, a.grid.human_xy.bytes(), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(a.grid.robot_xy.p, b.robot_xy, a.grid.robot_xy.bytes(), hipMemcpyDeviceToDevice, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(sc.dev.p, b.human_xy, grid_block(E, N, F, nullptr, nullptr), hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, launch_scene(g, h->stream));
    sc.n_in.resize(E);
    char* const pout = pin + pin_in;
    if (host) {
        // the download block in one copy: every array sits in the pinned block where it sits behind n_in on the device
        const auto back = [&](const auto& arr) { return pout + ((const char*)arr.p - (const char*)a.n_in.p); };
        HIPCHK(h, hipMemcpyAsync(pout, a.n_in.p, a.down_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::memcpy(sc.n_in.data(), pout, b_nin);
        std::memcpy(b.n_in_out, pout, b_nin);
        std::memcpy(b.in_cluster_out, back(a.in_cluster), a.in_cluster.bytes());
        std::memcpy(b.robot_in_cluster_out, back(a.robot_in), a.robot_in.bytes());
        if (b.cv_out) std::memcpy(b.cv_out, back(a.cv), a.cv.bytes());
    } else {
        HIPCHK(h, hipMemcpyAsync(pout, a.n_in.p, b_nin, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.n_in_out, a.n_in.p, b_nin, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.in_cluster_out, a.in_cluster.p, a.in_cluster.bytes(), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.robot_in_cluster_out, a.robot_in.p, a.robot_in.bytes(), hipMemcpyDeviceToDevice, h->stream));
        if (b.cv_out) HIPCHK(h, hipMemcpyAsync(b.cv_out, a.cv.p, a.cv.bytes(), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::memcpy(sc.n_in.data(), pout, b_nin);
    }
    sc.arr = a;
    sc.stamped = b.src == SCENE_DEVICE_GRID;
    sc.horizon = horizon;
    sc.E = E; sc.N = N;
    return 0;
}

// the refusals jmid_predict_scene and jmid_forecast_scene share
int check_predict_scene(jmid_ctx* h, const ChainCall& c) {
    const std::string who(c.who);
    const int E = c.E, A = c.A, K = c.K, T = c.T;
    if (int rc = check_ready(h)) return rc;
    if (E <= 0 || A <= 0 || K <= 0 || T <= 0 || c.k < 1 || c.k > K) return fail(h, JMID_EINVAL, who + ": bad dimensions");
    if (c.seeded ? !c.seeded->ids : !c.x_T) return fail(h, JMID_EINVAL, who + ": null input");            // x_T, or the episode ids of a seeded call
    const jmid_ctx::SceneWs& sc = h->scene;
    if (!sc.E) return fail(h, JMID_EINVAL, who + " needs a preceding jmid_build_scene on this handle");
    if (E != sc.E) return fail(h, JMID_EINVAL, who + ": E differs from the resident scene's");
    if (c.padded) {      // A is the largest count of the scene, and nobody's cluster is empty
        int most = 0;
        for (int e = 0; e < E; ++e) {
            if (sc.n_in[e] < 1) return fail(h, JMID_EINVAL, who + ": episode " + std::to_string(e) + " has no in-cluster pedestrian");
            most = std::max(most, sc.n_in[e]);
        }
        if (most != A)
            return fail(h, JMID_EINVAL, who + ": A = " + std::to_string(A) + " is not the largest in-cluster count of the resident scene, " + std::to_string(most));
    }
    for (int e = 0; e < E && !c.padded; ++e)
        if (sc.n_in[e] != A)
            return fail(h, JMID_EINVAL, who + ": episode " + std::to_string(e) + " has " + std::to_string(sc.n_in[e]) +
                                            " in-cluster pedestrians, not A = " + std::to_string(A) + " (group the episodes by their count)");
    if (c.rank() && (A > 32 || K > 1024 || T > 24)) return fail(h, JMID_EINVAL, who + ": the device top-k supports A <= 32, K <= 1024, T <= 24");
    if (h->ddpm) return fail(h, JMID_EINVAL, who + " samples with DDIM (MID.eval_sicnav: sampling=\"ddim\", MID/mid.py:333)");
    return 0;
}

// jmid_predict_scene / jmid_forecast_scene, their seeded and their padded forms: one chain, the noise either the caller's x_T or (seed, ids);
// padded: mixed in-cluster counts, A the largest, in the layout of jmid_predict_padded.  The entry states forecast, padded, the noise and
// the outputs; scene mode and the resident scene's counts are filled in here
int predict_scene_entry(jmid_handle_t h, ChainCall c) {
    if (!h) return JMID_EINVAL;
    const std::string w(c.who);
    c.scene = true;
    if (int rc = check_predict_scene(h, c)) return rc;
    if (c.seeded && !noise_fits((unsigned long long)c.K * c.A * c.T * 2)) return fail(h, JMID_EINVAL, w + ": K * A * T exceeds the noise addressing");
    if (c.forecast) {
        if (!c.forecasts_out || !c.logw_out) return fail(h, JMID_EINVAL, w + ": null output");
        if (!h->scene.horizon) return fail(h, JMID_EINVAL, w + ": the resident scene was built without cv_out (the rows outside the cluster need it)");
        if (h->scene.horizon != c.T)
            return fail(h, JMID_EINVAL, w + ": T = " + std::to_string(c.T) + " differs from the horizon " + std::to_string(h->scene.horizon) +
                                            " the resident scene was built with");
    } else {
        if (c.rank() && (!c.sel || !c.logw)) return fail(h, JMID_EINVAL, w + ": k < K needs sel and logw");
        if (!c.rank() && !c.pos_out) return fail(h, JMID_EINVAL, w + ": k == K needs pos_out");
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (c.padded) c.n_agents = h->scene.n_in.data();
    return predict_chain(h, c);
}

// jmid_noise_fill_padded: every episode's own compact draw in the padded layout, quiet NaN in the padded rows
int noise_padded_entry(jmid_handle_t h, uint64_t seed, int E, int A, int K, int T, const int32_t* n_agents, const uint32_t* episode_ids, int draw,
                       float* out, int mem) {
    if (!h) return JMID_EINVAL;
    const char* who = "jmid_noise_fill_padded";
    const std::string w(who);
    if (E < 1 || A < 1 || K < 1 || T < 1 || draw < 0) return fail(h, JMID_EINVAL, w + ": E, A, K, T must be at least 1 and draw at least 0");
    if (!episode_ids || !out) return fail(h, JMID_EINVAL, w + ": null argument");
    if (int rc = check_n_agents(h, who, n_agents, E, A)) return rc;
    const size_t n = (size_t)K * A * T * 2;
    if (!noise_fits(n)) return fail(h, JMID_EINVAL, w + ": K * A * T exceeds the noise addressing");
    HIPCHK(h, hipSetDevice(h->device));
    float* dst = nullptr;
    Staging st(h, mem, h->kde_ws, who);
    st.out(&dst, out, (size_t)E * n);
    if (int rc = st.begin()) return rc;
    if (int rc = h->noise_ids.upload(h, episode_ids, E, who)) return rc;
    if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
    if (int rc = fill_noise_padded(h, seed, h->noise_ids.get<unsigned>(), h->nag.get<int>(), E, A, K, T, draw, dst, h->stream)) return rc;
    HIPCHK(h, launch_pad_fill(dst, h->nag.get<int>(), E, K, A, T * 2, std::numeric_limits<float>::quiet_NaN(), h->stream));
    return st.end();
}

// jmid_noise_fill and jmid_dbg_noise_words: one draw to the caller's buffer (normals or raw words; 4 bytes per element either way)
int noise_entry(jmid_handle_t h, const char* who, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, float* out,
                unsigned* words, int mem) {
    if (!h) return JMID_EINVAL;
    const std::string w(who);
    if (E < 1 || rows < 1 || T < 1 || draw < 0) return fail(h, JMID_EINVAL, w + ": E, rows, T must be at least 1 and draw at least 0");
    if (!episode_ids || (!out && !words)) return fail(h, JMID_EINVAL, w + ": null argument");
    const size_t n = (size_t)rows * T * 2;
    if (!noise_fits(n)) return fail(h, JMID_EINVAL, w + ": rows * T exceeds the noise addressing");
    HIPCHK(h, hipSetDevice(h->device));
    char* dst = nullptr;             // host mode: staged in the handle's second workspace (the arena may hold the last call's positions)
    Staging st(h, mem, h->kde_ws, who);
    st.out(&dst, out ? (char*)out : (char*)words, (size_t)E * n * 4);
    if (int rc = st.begin()) return rc;
    if (int rc = h->noise_ids.upload(h, episode_ids, E, who)) return rc;
    if (int rc = fill_noise(h, seed, h->noise_ids.get<unsigned>(), E, n, draw, out ? (float*)dst : nullptr, words ? (unsigned*)dst : nullptr, h->stream)) return rc;
    return st.end();
}

// The workspace of jmid_denoise_reject_seeded, laid out here only: the call's ctx and p0 (host mode: their uploads) | the accepted block |
// the rerun's input and output blocks | the flags' per-sample values | the tables | the download block of a round (the rerun list with its
// length in front, then the range flag).  base null: the size only
struct RejectIo {
    Arr<float> ctx, p0;                        // [E, A, ctx_dim] | [E, A, 2] (host mode)
    Arr<float> acc_vel, acc_pos;               // [E, K, A, T, 2] twice (acc_vel: when velocities are asked for)
    Arr<float> g_ctx, g_p0, cand_vel, cand_pos;      // a rerun of at most E episodes (none with max_rounds = 0)
    Arr<double> ws, ws_wall;                   // [E, K, 2] each (ws_wall: with walls)
    Arr<int> slots, episodes, remaining;       // [E, K, 3] | [E, 3] | [E]
    Arr<int> list, flag, cause;                // [1 + E] | one word | [E, 2]: the download block (the causes of round 0 ride along)
    size_t down_bytes = 0;
};
size_t reject_io(const jmid_ctx* h, int E, int A, int K, int T, bool host, bool vel, bool rerun, bool with_walls, char* base, RejectIo* out) {
    const size_t EA = (size_t)E * A, M2 = (size_t)E * K * A * T * 2, Er = rerun ? 1 : 0;
    Carver c(base);
    RejectIo io{};
    io.ctx = c.arr(host ? EA * h->ctx_dim : 0); io.p0 = c.arr(host ? EA * 2 : 0);
    io.acc_vel = c.arr(vel ? M2 : 0); io.acc_pos = c.arr(M2);
    io.g_ctx = c.arr(Er * EA * h->ctx_dim); io.g_p0 = c.arr(Er * EA * 2); io.cand_vel = c.arr(vel ? Er * M2 : 0); io.cand_pos = c.arr(Er * M2);
    io.ws = c.arr<double>((size_t)E * K * CLS_WS_COLS); io.ws_wall = c.arr<double>(with_walls ? (size_t)E * K * WLS_WS_COLS : 0);
    io.slots = c.arr<int>((size_t)E * K * REJ_SLOT_COLS); io.episodes = c.arr<int>((size_t)E * REJ_EPISODE_COLS); io.remaining = c.arr<int>(E);
    const size_t down = c.off;
    io.list = c.arr<int>((size_t)E + 1); io.flag = c.arr<int>(1); io.cause = c.arr<int>((size_t)E * 2);
    io.down_bytes = c.off - down;
    if (out) *out = io;
    return c.off;
}

// The walls of a rejection call: the segments on the device (upload_walls) and the radius; L = 0: no wall predicate
struct RejectWalls {
    int L = 0;
    const double* dev = nullptr;
    double radius = 0.0;
};

// jmid_denoise_reject_seeded (no walls) and jmid_denoise_reject_walls_seeded after their argument checks.  Every round is one seeded
// denoise call through run_network (a stage: no caller-stream ordering, the range flag comes with the round's one download), the flags of
// its candidates - the collision kernel and, with walls, the wall kernel next to it -, the pairing, the compaction.
int reject_loop(jmid_ctx* h, const char* who, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids, int draw0,
                const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds, const RejectWalls& walls, float* vel_out,
                float* pos_out, int32_t* slot_out, int32_t* episode_out, int32_t* cause_out, int mem) {
    const bool host = mem == JMID_MEM_HOST, vel = vel_out != nullptr, split = precision != JMID_PREC_F32, with_walls = walls.L > 0;
    h->last_pos = nullptr;
    if (int rc = order_in(h, mem)) return rc;
    if (int rc = h->reject_ws.reserve(h, reject_io(h, E, A, K, T, host, vel, max_rounds > 0, with_walls, nullptr, nullptr), who)) return rc;
    RejectIo io;
    reject_io(h, E, A, K, T, host, vel, max_rounds > 0, with_walls, h->reject_ws.p, &io);
    if (int rc = h->reject_pin.reserve(h, io.down_bytes, who)) return rc;
    const int* pin = h->reject_pin.as<int>();
    const size_t flag_word = (size_t)((const char*)io.flag.p - (const char*)io.list.p) / sizeof(int);
    if (host) {
        HIPCHK(h, hipMemcpyAsync(io.ctx.p, ctx, io.ctx.bytes(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(io.p0.p, p0, io.p0.bytes(), hipMemcpyHostToDevice, h->stream));
        ctx = io.ctx.p; p0 = io.p0.p;
    }
    HIPCHK(h, hipMemsetAsync(io.flag.p, 0, sizeof(int), h->stream));
    RejectArgs g{};
    g.ws = io.ws; g.ws_wall = io.ws_wall; g.cand_pos = io.cand_pos; g.cand_vel = io.cand_vel; g.acc_pos = io.acc_pos; g.acc_vel = io.acc_vel;
    g.slots = io.slots; g.episodes = io.episodes; g.remaining = io.remaining; g.cause = io.cause; g.list = io.list;
    g.ctx = ctx; g.p0 = p0; g.g_ctx = io.g_ctx; g.g_p0 = io.g_p0;
    g.E = E; g.K = K; g.n = A * T * 2; g.n_ctx = A * h->ctx_dim; g.n_p0 = A * 2;
    std::vector<uint32_t> ids(episode_ids, episode_ids + E);
    // a padded batch: the counts of the round's episodes, a host array the round's denoise call checks and uploads (h->nag); the flag
    // kernels behind it on the stream read that upload
    std::vector<int32_t> nag;
    if (n_agents) nag.assign(n_agents, n_agents + E);
    int n_run = E;
    for (int j = 0; j <= max_rounds && n_run > 0; ++j) {
        if (j > 0) {      // the listed episodes, ascending: their ids, their counts, their rows
            for (int b = 0; b < n_run; ++b) ids[b] = episode_ids[pin[1 + b]];
            for (int b = 0; b < n_run && n_agents; ++b) nag[b] = n_agents[pin[1 + b]];
            HIPCHK(h, launch_reject_gather(g, n_run, h->stream));
        }
        const SeedArgs sa{seed, ids.data(), draw0 + j};
        DenoiseCall d{n_run, A, K, T, precision, JMID_MEM_DEVICE};
        d.ctx = j ? io.g_ctx.p : ctx; d.p0 = j ? io.g_p0.p : p0; d.dt = dt; d.seeded = &sa; d.chained = true; d.who = who;
        d.vel_out = j ? io.cand_vel : io.acc_vel; d.pos_out = j ? io.cand_pos.p : io.acc_pos.p;      // round 0 IS the accepted block
        if (n_agents) d.n_agents = nag.data();       // (the row stride stays the call's A whatever counts are left)
        if (int rc = run_network(h, d)) return rc;
        h->last_pos = nullptr;       // (the arena's stage is not what pos = NULL means after this entry)
        const int* nag_dev = n_agents ? h->nag.get<int>() : nullptr;
        {
            ProfScope ps(h, KC_EVAL_STATS, h->stream);
            CollisionStatsArgs cs{};
            cs.pos = d.pos_out; cs.ws = io.ws; cs.threshold = threshold;
            cs.E = n_run; cs.A = A; cs.K = K; cs.T = T; cs.n_agents = nag_dev;
            HIPCHK(h, launch_collision_stats(cs, h->stream));
            if (with_walls) {
                WallStatsArgs ww{};
                ww.pos = d.pos_out; ww.p0 = d.p0; ww.walls = walls.dev; ww.ws = io.ws_wall; ww.radius = walls.radius;
                ww.E = n_run; ww.A = A; ww.K = K; ww.T = T; ww.L = walls.L; ww.n_agents = nag_dev;
                HIPCHK(h, launch_wall_stats(ww, h->stream));
            }
            g.round = j;
            HIPCHK(h, j ? launch_reject_accept(g, n_run, h->stream) : launch_reject_init(g, h->stream));
            HIPCHK(h, launch_reject_compact(g, h->stream));
        }
        // the round's one download: how many episodes the next round reruns and which, and the range flag of this round's denoise call
        if (split) HIPCHK(h, hipMemcpyAsync(io.flag.p, h->range_flag, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->reject_pin.p, io.list.p, io.down_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (split && pin[flag_word]) {
            (void)order_out(h, mem);
            return flagged_call(h, pin[flag_word]);
        }
        n_run = pin[0];
        if (n_run < 0 || n_run > E) return fail(h, JMID_EHIP, std::string(who) + ": the rerun list came back with an impossible length");
    }
    const hipMemcpyKind kout = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (vel_out) HIPCHK(h, hipMemcpyAsync(vel_out, io.acc_vel.p, io.acc_vel.bytes(), kout, h->stream));
    if (pos_out) HIPCHK(h, hipMemcpyAsync(pos_out, io.acc_pos.p, io.acc_pos.bytes(), kout, h->stream));
    if (slot_out) HIPCHK(h, hipMemcpyAsync(slot_out, io.slots.p, io.slots.bytes(), kout, h->stream));
    if (episode_out) HIPCHK(h, hipMemcpyAsync(episode_out, io.episodes.p, io.episodes.bytes(), kout, h->stream));
    if (cause_out) {      // host mode: the causes came with the rounds' download - no copy of their own
        if (host) std::memcpy(cause_out, pin + ((const char*)io.cause.p - (const char*)io.list.p) / sizeof(int), io.cause.bytes());
        else HIPCHK(h, hipMemcpyAsync(cause_out, io.cause.p, io.cause.bytes(), kout, h->stream));
    }
    if (host) HIPCHK(h, hipStreamSynchronize(h->stream));
    // the accepted set is what pos = NULL consumers see, under jmid_denoise's forgetting rules (every later denoise call and every
    // host-mode entry that clears last_pos forgets it, although this block itself would survive them)
    h->last_pos = io.acc_pos.p;
    h->last_vel = io.acc_vel; h->last_vel_pos = io.acc_pos.p;
    h->last_pos_dims[0] = E; h->last_pos_dims[1] = A; h->last_pos_dims[2] = K; h->last_pos_dims[3] = T;
    return order_out(h, mem);
}

}  // namespace jmid_host

// What the handle created, and only that: a handle that never created anything (jmid_dbg_plan_chunks_mode builds one on the stack) makes
// no HIP call here.  The member owners (the workspaces, the id / count arrays) free themselves after this body.
jmid_ctx::~jmid_ctx() {
    drop_graphs(this);
    free_weights(this);
    for (int c = 0; c < KC_COUNT; ++c) ev_pool.insert(ev_pool.end(), prof_ev[c].begin(), prof_ev[c].end());
    for (auto& ev : ev_pool) {
        hipEventDestroy(ev.a);
        hipEventDestroy(ev.b);
    }
    for (int l = 0; l < kMaxLanes - 1; ++l) {
        if (lane_stream[l]) hipStreamDestroy(lane_stream[l]);
        if (ev_join[l]) hipEventDestroy(ev_join[l]);
    }
    if (stream) hipStreamDestroy(stream);
    for (hipEvent_t e : {ev_in, ev_out, ev_fork})
        if (e) hipEventDestroy(e);
}

// ================================================================================================ C ABI
extern "C" {

const char* jmid_version(void) {
#ifdef JMID_DIAGNOSTICS
    return "jmid_hip 0.7.0+diagnostics (gfx950; f32-mfma + f16x3 / f16x2 split-mfma + f16mx fp8-correction)";
#else
    return "jmid_hip 0.7.0 (gfx950; f32-mfma + f16x3 / f16x2 split-mfma + f16mx fp8-correction)";
#endif
}

int jmid_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* jmid_last_error(jmid_handle_t h) { return h ? h->err.c_str() : thread_error().c_str(); }

int jmid_create(jmid_handle_t* out, int device_id, int net_kind, int ctx_dim, int tf_layer, int nhead, int hist_len) {
    if (!out) return JMID_EINVAL;
    *out = nullptr;
    if (net_kind != JMID_NET_IMID && net_kind != JMID_NET_JMID) return fail(nullptr, JMID_EINVAL, "bad net_kind");
    if (ctx_dim < 32 || ctx_dim % 32 != 0 || ctx_dim > 512)
        return fail(nullptr, JMID_EINVAL, "ctx_dim must be a multiple of 32 in [32, 512]");
    if (tf_layer < 1 || tf_layer > 16) return fail(nullptr, JMID_EINVAL, "bad tf_layer");
    const int d = 2 * ctx_dim;
    if (nhead < 1 || d % nhead != 0) return fail(nullptr, JMID_EINVAL, "nhead must divide d_model");
    const int hd = d / nhead;
    if (hd != 16 && hd != 32 && hd != 64 && hd != 128)
        return fail(nullptr, JMID_EINVAL, "head_dim must be one of 16, 32, 64, 128");
    if (hist_len < 1 || hist_len > ENC_MAX_TH) return fail(nullptr, JMID_EINVAL, "hist_len out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, JMID_EHIP, "no HIP device available (libjmid_hip has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, JMID_EINVAL, "device_id out of range");
    jmid_ctx* h = new jmid_ctx();
    h->device = device_id;
    h->net_kind = net_kind;
    h->ctx_dim = ctx_dim;
    h->tf_layer = tf_layer;
    h->nhead = nhead;
    h->hist_len = hist_len;
    h->d = d;
    h->ff = 4 * ctx_dim;
    h->dmid = ctx_dim;
    h->dlow = ctx_dim / 2;
    h->H = ctx_dim / 2;
    h->hl = make_hyper_layout(h->d, h->dmid, h->dlow);
    register_shapes(h);
    // NON-BLOCKING streams: a blocking stream is implicitly ordered against the legacy null stream, so once ANYTHING in the process
    // (torch on its default stream, or this handle's own device-mode ordering events) has put work on the null stream, every launch on
    // the handle's stream pays for that coupling - one cfg2 call went from 10.1 to 13.0 ms after a single device-mode call on the handle
    // (tools/predict_probe.py).  The handle orders itself against the caller's stream EXPLICITLY (order_in / order_out: events), host-mode
    // calls synchronise the stream before they return, and nothing in the library uses the null stream.
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) == hipSuccess;
    for (int l = 0; ok && l < jmid_ctx::kMaxLanes - 1; ++l)
        ok = hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        delete h;       // (~jmid_ctx: the streams and events that do exist)
        return fail(nullptr, JMID_EHIP, "cannot create a HIP stream");
    }
    // compute units of this device (or of its partition): the kernels whose workgroups wait for each other launch only when all of
    // them are resident at once (gemm_small.hpp::small_lnx_fits)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) h->tune.cus = cus;
    *out = h;
    return JMID_OK;
}

int jmid_destroy(jmid_handle_t h) {
    if (!h) return JMID_OK;
    hipSetDevice(h->device);
    sync_lanes(h);
    drop_graphs(h);
    delete h;
    return JMID_OK;
}

int jmid_denoise_ddpm(jmid_handle_t h, int E, int A, int K, int T, const float* x_T, const float* z, const float* ctx,
                      const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!z) return fail(h, JMID_EINVAL, "null z");
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x_T; c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out; c.z = z; c.who = "jmid_denoise_ddpm";
    return run_network(h, c);
}

// jmid_encode (first_index null: the launch it always made) and jmid_encode_var (a HOST array, refused here before anything is enqueued)
static int encode_entry(jmid_handle_t h, const char* who, int n_agents, const float* x_st, const float* nbr_sum, const float* edge_mask,
                        const int32_t* first_index, float* ctx_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!h->finalized) return fail(h, JMID_ENOWEIGHT, "jmid_finalize_weights has not been called");
    if (n_agents <= 0 || !x_st || !nbr_sum || !edge_mask || !ctx_out) return fail(h, JMID_EINVAL, "bad argument");
    if (first_index)
        for (int r = 0; r < n_agents; ++r)
            if (first_index[r] < 0 || first_index[r] > h->hist_len - 2)
                return fail(h, JMID_EINVAL, std::string(who) + ": first_index[" + std::to_string(r) + "] = " + std::to_string(first_index[r]) +
                                                " is outside 0..hist_len-2 (a row needs two history frames)");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = n_agents, Th = h->hist_len;
    EncArgs ea = encoder_args(h, nullptr, nullptr, nullptr, nullptr, n_agents);
    if (mem == JMID_MEM_HOST) h->last_pos = nullptr;      // the staging below overwrites the workspace the last positions live in
    Staging st(h, mem, h->arena, who);
    st.in(&ea.x_st, x_st, n * Th * 6);
    st.in(&ea.nbr_sum, nbr_sum, n * 2 * Th * 6);
    st.in(&ea.edge_mask, edge_mask, n * 2);
    st.out(&ea.ctx, ctx_out, n * 2 * h->H);
    if (int rc = st.begin()) return rc;
    if (first_index) {
        if (int rc = h->first_idx.upload(h, first_index, n_agents, who)) return rc;
        ea.first_index = h->first_idx.get<int>();
    }
    {
        ProfScope ps(h, KC_ENCODER, h->stream);
        HIPCHK(h, launch_encoder(ea, h->stream));
    }
    return st.end();
}

int jmid_encode(jmid_handle_t h, int n_agents, const float* x_st, const float* nbr_sum, const float* edge_mask,
                float* ctx_out, int mem) {
    return encode_entry(h, "jmid_encode", n_agents, x_st, nbr_sum, edge_mask, nullptr, ctx_out, mem);
}

int jmid_encode_var(jmid_handle_t h, int n_agents, const float* x_st, const float* nbr_sum, const float* edge_mask,
                    const int32_t* first_index, float* ctx_out, int mem) {
    if (h && !first_index) return fail(h, JMID_EINVAL, "jmid_encode_var: null first_index");
    return encode_entry(h, "jmid_encode_var", n_agents, x_st, nbr_sum, edge_mask, first_index, ctx_out, mem);
}

int jmid_denoise(jmid_handle_t h, int E, int A, int K, int T, const float* x_T, const float* ctx, const float* p0,
                 float dt, int precision, float* vel_out, float* pos_out, int mem) {
    if (!h) return JMID_EINVAL;
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x_T; c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out;
    return run_network(h, c);
}

int jmid_net_eval(jmid_handle_t h, int E, int A, int K, int T, int step_idx, const float* x, const float* ctx,
                  int precision, float* e_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!e_out) return fail(h, JMID_EINVAL, "null e_out");
    if (int rc = check_ready(h)) return rc;
    if (step_idx < 0 || step_idx >= (int)h->beta.size()) return fail(h, JMID_EINVAL, "step_idx out of range");
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x; c.ctx = ctx; c.e_out = e_out; c.single_step = step_idx; c.who = "jmid_net_eval";
    return run_network(h, c);
}

int jmid_net_eval_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, int step_idx, const float* x, const float* ctx,
                         int precision, float* e_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!n_agents) return fail(h, JMID_EINVAL, "jmid_net_eval_padded: null n_agents");
    if (!e_out) return fail(h, JMID_EINVAL, "null e_out");
    if (int rc = check_ready(h)) return rc;
    if (step_idx < 0 || step_idx >= (int)h->beta.size()) return fail(h, JMID_EINVAL, "step_idx out of range");
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x; c.ctx = ctx; c.e_out = e_out; c.single_step = step_idx; c.n_agents = n_agents; c.who = "jmid_net_eval_padded";
    return run_network(h, c);
}

// jmid_loss (seeded null) and jmid_loss_seeded: one net evaluation with K = 1 at per-row timesteps, the squared error against e reduced on
// the device (loss.hpp).  Every argument error surfaces in check_call, before anything is enqueued.
static int loss_entry(jmid_handle_t h, const char* who, int E, int A, int T, const int32_t* n_agents, const int32_t* t, const float* x0, const float* e,
                      const SeedArgs* seeded, const float* ctx, int precision, double* loss_out, double* row_out, float* e_theta_out, int mem) {
    if (!h) return JMID_EINVAL;
    LossCall lc;
    lc.t = t; lc.e = e; lc.seeded = seeded; lc.loss_out = loss_out; lc.row_out = row_out;
    DenoiseCall c{E, A, 1, T, precision, mem};
    c.x_in = x0; c.ctx = ctx; c.e_out = e_theta_out; c.single_step = 0; c.n_agents = n_agents; c.loss = &lc; c.who = who;
    return run_network(h, c);
}

int jmid_loss(jmid_handle_t h, int E, int A, int T, const int32_t* n_agents, const int32_t* t, const float* x0, const float* e, const float* ctx,
              int precision, double* loss_out, double* row_out, float* e_theta_out, int mem) {
    if (h && !e) return fail(h, JMID_EINVAL, "jmid_loss: null e");
    return loss_entry(h, "jmid_loss", E, A, T, n_agents, t, x0, e, nullptr, ctx, precision, loss_out, row_out, e_theta_out, mem);
}

int jmid_loss_seeded(jmid_handle_t h, int E, int A, int T, const int32_t* n_agents, const int32_t* t, const float* x0, uint64_t seed,
                     const uint32_t* episode_ids, const float* ctx, int precision, double* loss_out, double* row_out, float* e_theta_out, int mem) {
    const SeedArgs sa{seed, episode_ids};
    return loss_entry(h, "jmid_loss_seeded", E, A, T, n_agents, t, x0, nullptr, &sa, ctx, precision, loss_out, row_out, e_theta_out, mem);
}

int jmid_denoise_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x_T, const float* ctx, const float* p0,
                        float dt, int precision, float* vel_out, float* pos_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!n_agents) return fail(h, JMID_EINVAL, "jmid_denoise_padded: null n_agents");
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x_T; c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out; c.n_agents = n_agents; c.who = "jmid_denoise_padded";
    return run_network(h, c);
}

int jmid_episode_metrics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt,
                         float* out, int mem) {
    if (!h || !pos || !gt || !out || E <= 0 || A <= 0 || K <= 0 || T <= 0) return fail(h, JMID_EINVAL, "bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    const float *dp, *dg;
    float* dout;
    if (mem == JMID_MEM_HOST) h->last_pos = nullptr;      // (as in jmid_encode)
    Staging st(h, mem, h->arena, "jmid_episode_metrics");
    st.in(&dp, pos, (size_t)E * K * A * T * 2);
    st.in(&dg, gt, (size_t)E * A * T * 2);
    st.out(&dout, out, (size_t)E * 4);
    if (int rc = st.begin()) return rc;
    if (int rc = launch_episode_metrics(h, dp, dg, dout, E, K, A, T)) return rc;
    return st.end();
}

int jmid_eval_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt, float* agent_out,
                         float* scene_out, int mem) {
    if (!h || !gt || !agent_out || E <= 0 || A <= 0 || T <= 0) return fail(h, JMID_EINVAL, "bad argument");
    if (K < 2 || K > 1024 || T > 24) return fail(h, JMID_EINVAL, "jmid_eval_statistics supports 2 <= K <= 1024, T <= 24");
    if ((size_t)E * A > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, "jmid_eval_statistics: E * A exceeds the launch grid");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    EvalStatsArgs g{};
    g.E = E; g.A = A; g.K = K; g.T = T;
    Staging st(h, mem, h->kde_ws, "jmid_eval_statistics");
    st.in(&g.gt, gt, (size_t)E * A * T * 2);
    if (pos) st.in(&g.pos, pos, (size_t)E * K * A * T * 2);
    else g.pos = h->last_pos;
    st.out(&g.agent_out, agent_out, (size_t)E * A * EVS_AGENT_COLS);
    if (scene_out) st.out(&g.scene_out, scene_out, (size_t)E * EVS_SCENE_COLS);
    if (int rc = st.begin()) return rc;
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_eval_stats(g, h->stream));
    }
    return st.end();
}

int jmid_eval_statistics_masked(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt,
                                const uint8_t* interp_future, const uint8_t* skip, int n_cut, const int* cutoffs, float* agent_out,
                                float* cut_out, float* scene_out, int mem) {
    if (!h || !gt || !interp_future || !agent_out || E <= 0 || A <= 0 || T <= 0) return fail(h, JMID_EINVAL, "bad argument");
    if (K < 2 || K > 1024 || T > 24) return fail(h, JMID_EINVAL, "jmid_eval_statistics_masked supports 2 <= K <= 1024, T <= 24");
    if ((size_t)E * A > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, "jmid_eval_statistics_masked: E * A exceeds the launch grid");
    if (n_cut < 0 || n_cut > EVS_MAX_CUTS || (n_cut > 0 && (!cutoffs || !cut_out)))
        return fail(h, JMID_EINVAL, "jmid_eval_statistics_masked takes 0 <= n_cut <= 4 cut-offs (with cutoffs and cut_out)");
    EvalStatsMaskedArgs g{};
    for (int j = 0; j < n_cut; ++j) {
        if (cutoffs[j] < 0 || cutoffs[j] >= T) return fail(h, JMID_EINVAL, "jmid_eval_statistics_masked: a cut-off step is not in [0, T)");
        g.cutoffs[j] = cutoffs[j];
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    g.E = E; g.A = A; g.K = K; g.T = T; g.n_cut = n_cut;
    Staging st(h, mem, h->kde_ws, "jmid_eval_statistics_masked");
    st.in(&g.gt, gt, (size_t)E * A * T * 2);
    st.in(&g.interp, interp_future, (size_t)E * A * T);
    if (skip) st.in(&g.skip, skip, (size_t)E * A);
    if (pos) st.in(&g.pos, pos, (size_t)E * K * A * T * 2);
    else g.pos = h->last_pos;
    st.out(&g.agent_out, agent_out, (size_t)E * A * EVS_MASKED_AGENT_COLS);
    if (n_cut) st.out(&g.cut_out, cut_out, (size_t)E * A * n_cut * EVS_CUT_COLS);
    if (scene_out) st.out(&g.scene_out, scene_out, (size_t)E * EVS_SCENE_COLS);
    if (int rc = st.begin()) return rc;
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_eval_stats_masked(g, h->stream));
    }
    return st.end();
}

// jmid_collision_statistics (n_agents null) and jmid_collision_statistics_padded (a HOST array, checked by the entry)
static int collision_entry(jmid_handle_t h, const char* who, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, double threshold,
                           float* pair_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem) {
    if (!h || E <= 0) return fail(h, JMID_EINVAL, "bad argument");
    const std::string w(who);
    if (K < 1 || K > CLS_MAX_K || T < 2 || T > CLS_MAX_T || A < 1 || A > CLS_MAX_A)
        return fail(h, JMID_EINVAL, w + " supports 1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(h, JMID_EINVAL, w + ": the threshold must be finite and >= 0");
    if (!pair_out && !agent_out && !sample_out && !scene_out) return fail(h, JMID_EINVAL, w + ": every output is NULL");
    if ((size_t)E * K > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, w + ": E * K exceeds the launch grid");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    const size_t P = (size_t)A * (A - 1) / 2;
    CollisionStatsArgs g{};
    g.E = E; g.A = A; g.K = K; g.T = T;
    g.threshold = threshold;
    Staging st(h, mem, h->kde_ws, who);
    st.scratch(&g.ws, (size_t)E * K * CLS_WS_COLS * 8);      // the per-sample fp64 values the scene kernel reduces
    if (pos) st.in(&g.pos, pos, (size_t)E * K * A * T * 2);
    else g.pos = h->last_pos;
    if (pair_out) st.out(&g.pair_out, pair_out, (size_t)E * K * P);
    if (agent_out) st.out(&g.agent_out, agent_out, (size_t)E * K * A);
    if (sample_out) st.out(&g.sample_out, sample_out, (size_t)E * K * CLS_SAMPLE_COLS);
    if (scene_out) st.out(&g.scene_out, scene_out, (size_t)E * CLS_SCENE_COLS);
    if (int rc = st.begin()) return rc;
    if (n_agents) {
        if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
        g.n_agents = h->nag.get<int>();
    }
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_collision_stats(g, h->stream));
    }
    return st.end();
}

int jmid_collision_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, double threshold, float* pair_out,
                              uint8_t* agent_out, float* sample_out, float* scene_out, int mem) {
    return collision_entry(h, "jmid_collision_statistics", E, A, K, T, nullptr, pos, threshold, pair_out, agent_out, sample_out, scene_out, mem);
}

int jmid_collision_statistics_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, double threshold,
                                     float* pair_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (E > 0 && A > 0)
        if (int rc = check_n_agents(h, "jmid_collision_statistics_padded", n_agents, E, A)) return rc;
    return collision_entry(h, "jmid_collision_statistics_padded", E, A, K, T, n_agents, pos, threshold, pair_out, agent_out, sample_out, scene_out, mem);
}

// jmid_wall_statistics (n_agents null) and jmid_wall_statistics_padded (a HOST array, checked by the entry)
static int wall_entry(jmid_handle_t h, const char* who, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, int L,
                      const double* walls, double radius, float* dist_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem) {
    if (!h || E <= 0) return fail(h, JMID_EINVAL, "bad argument");
    const std::string w(who);
    if (K < 1 || K > CLS_MAX_K || T < 2 || T > CLS_MAX_T || A < 1 || A > CLS_MAX_A)
        return fail(h, JMID_EINVAL, w + " supports 1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64");
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(h, JMID_EINVAL, w + ": the radius must be finite and >= 0");
    if (!dist_out && !agent_out && !sample_out && !scene_out) return fail(h, JMID_EINVAL, w + ": every output is NULL");
    if ((size_t)E * K > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, w + ": E * K exceeds the launch grid");
    HIPCHK(h, hipSetDevice(h->device));
    WallStatsArgs g{};
    if (int rc = upload_walls(h, L, walls, &g.walls, w)) return rc;
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    g.E = E; g.A = A; g.K = K; g.T = T; g.L = L;
    g.radius = radius;
    Staging st(h, mem, h->kde_ws, who);
    st.scratch(&g.ws, (size_t)E * K * WLS_WS_COLS * 8);      // the per-sample fp64 values the scene kernel reduces
    if (pos) st.in(&g.pos, pos, (size_t)E * K * A * T * 2);
    else g.pos = h->last_pos;
    if (p0) st.in(&g.p0, p0, (size_t)E * A * 2);
    if (dist_out && L > 0) st.out(&g.dist_out, dist_out, (size_t)E * K * A * L);
    if (agent_out) st.out(&g.agent_out, agent_out, (size_t)E * K * A);
    if (sample_out) st.out(&g.sample_out, sample_out, (size_t)E * K * WLS_SAMPLE_COLS);
    if (scene_out) st.out(&g.scene_out, scene_out, (size_t)E * WLS_SCENE_COLS);
    if (int rc = st.begin()) return rc;
    if (n_agents) {
        if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
        g.n_agents = h->nag.get<int>();
    }
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_wall_stats(g, h->stream));
    }
    return st.end();
}

int jmid_wall_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* p0, int L, const double* walls,
                         double radius, float* dist_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem) {
    return wall_entry(h, "jmid_wall_statistics", E, A, K, T, nullptr, pos, p0, L, walls, radius, dist_out, agent_out, sample_out, scene_out, mem);
}

int jmid_wall_statistics_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, int L,
                                const double* walls, double radius, float* dist_out, uint8_t* agent_out, float* sample_out, float* scene_out,
                                int mem) {
    if (!h) return JMID_EINVAL;
    if (E > 0 && A > 0)
        if (int rc = check_n_agents(h, "jmid_wall_statistics_padded", n_agents, E, A)) return rc;
    return wall_entry(h, "jmid_wall_statistics_padded", E, A, K, T, n_agents, pos, p0, L, walls, radius, dist_out, agent_out, sample_out, scene_out, mem);
}

// What the repair entries and a constrained chain with repair refuse alike: the shape limits and the conditions on the rule's arguments
// (with_p0: the call has a p0, so the velocities divide by dt)
static int repair_check(jmid_handle_t h, const std::string& w, bool with_walls, int E, int A, int K, int T, bool with_p0, float dt, double threshold,
                        double margin, double tau, double step, int max_iter, double wall_radius) {
    if (K < 1 || K > CLS_MAX_K || T < 2 || T > CLS_MAX_T || A < 1 || A > CLS_MAX_A)
        return fail(h, JMID_EINVAL, w + " supports 1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(h, JMID_EINVAL, w + ": the threshold must be finite and >= 0");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(h, JMID_EINVAL, w + ": the margin must be finite and >= 0");
    if (!(tau > 0.0) || !std::isfinite(tau)) return fail(h, JMID_EINVAL, w + ": tau must be finite and > 0");
    if (!(step > 0.0) || !std::isfinite(step)) return fail(h, JMID_EINVAL, w + ": the step must be finite and > 0");
    if (max_iter < 0 || max_iter > RPR_MAX_ITER) return fail(h, JMID_EINVAL, w + ": max_iter must lie in 0..1024");
    if (with_p0 && !(dt > 0.0f && std::isfinite(dt))) return fail(h, JMID_EINVAL, w + ": p0 needs a finite dt > 0 (the velocities divide by it)");
    if ((size_t)E * K > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, w + ": E * K exceeds the launch grid");
    if (with_walls && (!(wall_radius >= 0.0) || !std::isfinite(wall_radius))) return fail(h, JMID_EINVAL, w + ": the wall_radius must be finite and >= 0");
    return 0;
}

// The repair of colliding samples (repair.hpp): the collision kernel's lean form for the flags, the repair kernel, the episode rows - three
// launches on the handle's stream, nothing comes back to the host in between.  pos null: the resident set, in place.
// jmid_repair_collisions (with_walls false: L = 0, no wall_out) and jmid_repair_collisions_walls: with L > 0 the wall kernel's lean form runs
// next to the collision kernel's and the repair kernel is the instance with the wall terms - four launches
static int repair_entry(jmid_handle_t h, const char* who, bool with_walls, int E, int A, int K, int T, const int32_t* n_agents, const float* pos,
                        const float* p0, float dt, double threshold, double margin, double tau, double step, int max_iter, int L, const double* walls,
                        double wall_radius, float* pos_out, float* vel_out, float* sample_out, int32_t* episode_out, float* wall_out, int mem) {
    if (!h || E <= 0) return fail(h, JMID_EINVAL, "bad argument");
    const std::string w(who);
    if (int rc = repair_check(h, w, with_walls, E, A, K, T, p0 != nullptr, dt, threshold, margin, tau, step, max_iter, wall_radius)) return rc;
    if (vel_out && !p0) return fail(h, JMID_EINVAL, w + ": vel_out needs p0 (a velocity's first step starts at the present position)");
    if (pos && !pos_out && !vel_out && !sample_out && !episode_out && !wall_out) return fail(h, JMID_EINVAL, w + ": every output is NULL");
    if (n_agents)
        if (int rc = check_n_agents(h, who, n_agents, E, A)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    WallStatsArgs ws{};
    if (with_walls)
        if (int rc = upload_walls(h, L, walls, &ws.walls, w)) return rc;
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    const bool host = mem == JMID_MEM_HOST;
    const size_t M2 = (size_t)E * K * A * T * 2;
    CollisionStatsArgs cs{};
    cs.E = E; cs.A = A; cs.K = K; cs.T = T; cs.threshold = threshold;
    RepairWallArgs g{};
    g.E = E; g.A = A; g.K = K; g.T = T; g.max_iter = max_iter;
    g.threshold = threshold; g.margin = margin; g.tau = tau; g.step = step; g.dt = (double)dt;
    g.L = L; g.walls = ws.walls; g.wall_radius = wall_radius;
    ws.E = E; ws.A = A; ws.K = K; ws.T = T; ws.L = L; ws.radius = wall_radius;
    Staging st(h, mem, h->kde_ws, who);
    const size_t lean = (size_t)E * K * CLS_WS_COLS;          // the collision kernel's lean form, and behind it the wall kernel's (one slot)
    st.scratch(&cs.ws, (lean + (L > 0 ? (size_t)E * K * WLS_WS_COLS : 0)) * 8);
    if (pos) {
        st.in(&g.src, pos, M2);
        if (pos_out) st.out(&g.dst, pos_out, M2);
    } else {      // in place where the samples lie; pos_out is a copy of the block afterwards
        g.src = h->last_pos;
        g.dst = const_cast<float*>(h->last_pos);
        if (p0 && h->last_vel && h->last_vel_pos == h->last_pos) g.vel2 = h->last_vel;
    }
    if (p0 && (vel_out || g.vel2 || L > 0)) st.in(&g.p0, p0, (size_t)E * A * 2);      // (with walls: the first point of every path)
    if (vel_out) {      // in and out: only the rows of repaired samples are rewritten
        g.vel = vel_out;
        if (host) st.add(&g.vel, vel_out, vel_out, M2 * sizeof(float));
    }
    if (sample_out) st.out(&g.sample, sample_out, (size_t)E * K * RPR_SAMPLE_COLS);
    else st.scratch(&g.sample, (size_t)E * K * RPR_SAMPLE_COLS * sizeof(float));
    if (episode_out) st.out(&g.episode, episode_out, (size_t)E * RPR_EPISODE_COLS);
    if (wall_out) st.out(&g.wall_out, wall_out, (size_t)E * K * RPR_WALL_COLS);
    if (int rc = st.begin()) return rc;
    if (n_agents) {
        if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
        cs.n_agents = ws.n_agents = g.n_agents = h->nag.get<int>();
    }
    cs.pos = ws.pos = g.src;
    ws.p0 = g.p0;
    ws.ws = L > 0 ? cs.ws + lean : nullptr;
    g.ws = cs.ws;
    g.wws = ws.ws;
    {
        ProfScope ps(h, KC_EVAL_STATS, h->stream);
        HIPCHK(h, launch_collision_stats(cs, h->stream));
        if (!with_walls) {
            HIPCHK(h, launch_repair(g, h->stream));
        } else {
            if (L > 0) HIPCHK(h, launch_wall_stats(ws, h->stream));
            HIPCHK(h, launch_repair_walls(g, h->stream));
        }
    }
    if (!pos && pos_out) HIPCHK(h, hipMemcpyAsync(pos_out, h->last_pos, M2 * sizeof(float), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    return st.end();
}

int jmid_repair_collisions(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, float dt,
                           double threshold, double margin, double tau, double step, int max_iter, float* pos_out, float* vel_out,
                           float* sample_out, int32_t* episode_out, int mem) {
    return repair_entry(h, "jmid_repair_collisions", false, E, A, K, T, n_agents, pos, p0, dt, threshold, margin, tau, step, max_iter, 0, nullptr, 0.0,
                        pos_out, vel_out, sample_out, episode_out, nullptr, mem);
}

int jmid_repair_collisions_walls(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, float dt,
                                 double threshold, double margin, double tau, double step, int max_iter, int L, const double* walls,
                                 double wall_radius, float* pos_out, float* vel_out, float* sample_out, int32_t* episode_out, float* wall_out,
                                 int mem) {
    return repair_entry(h, "jmid_repair_collisions_walls", true, E, A, K, T, n_agents, pos, p0, dt, threshold, margin, tau, step, max_iter, L, walls,
                        wall_radius, pos_out, vel_out, sample_out, episode_out, wall_out, mem);
}

// What jmid_guide_step and the guided denoise entries refuse alike: the repair entries' conditions on threshold, margin, tau and
// wall_radius, n_inner, the shape limits (T = 1 is allowed: no pedestrian segment, the wall terms of the step from p0 only)
static int guide_check(jmid_handle_t h, const std::string& w, int E, int A, int K, int T, const float* p0, float dt, double threshold, double margin,
                       double tau, int n_inner, double wall_radius) {
    if (E <= 0) return fail(h, JMID_EINVAL, w + ": bad argument");
    if (K < 1 || K > CLS_MAX_K || T < 1 || T > CLS_MAX_T || A < 1 || A > CLS_MAX_A)
        return fail(h, JMID_EINVAL, w + " supports 1 <= K <= 1024, 1 <= T <= 24, 1 <= A <= 64");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(h, JMID_EINVAL, w + ": the threshold must be finite and >= 0");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(h, JMID_EINVAL, w + ": the margin must be finite and >= 0");
    if (!(tau > 0.0) || !std::isfinite(tau)) return fail(h, JMID_EINVAL, w + ": tau must be finite and > 0");
    if (n_inner < 1 || n_inner > GDE_MAX_INNER) return fail(h, JMID_EINVAL, w + ": n_inner must lie in 1..64");
    if (!(wall_radius >= 0.0) || !std::isfinite(wall_radius)) return fail(h, JMID_EINVAL, w + ": the wall_radius must be finite and >= 0");
    if (!p0) return fail(h, JMID_EINVAL, w + ": null p0 (the guidance is defined on positions)");
    if (!(dt > 0.0f) || !std::isfinite(dt)) return fail(h, JMID_EINVAL, w + ": dt must be finite and > 0");
    if ((size_t)E * K > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, w + ": E * K exceeds the launch grid");
    return 0;
}

// One application of the guidance rule (guide.hpp) to a block of velocities: what a guided denoise call runs behind one step-table entry
int jmid_guide_step(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x, const float* p0, float dt,
                    double threshold, double margin, double tau, double weight, int n_inner, int L, const double* walls, double wall_radius,
                    float* x_out, float* guide_out, int mem) {
    if (!h) return JMID_EINVAL;
    const char* who = "jmid_guide_step";
    const std::string w(who);
    if (int rc = guide_check(h, w, E, A, K, T, p0, dt, threshold, margin, tau, n_inner, wall_radius)) return rc;
    if (!(weight >= 0.0) || !std::isfinite(weight)) return fail(h, JMID_EINVAL, w + ": the weight must be finite and >= 0");
    if (!x || !x_out) return fail(h, JMID_EINVAL, w + ": null x / x_out");
    if (n_agents)
        if (int rc = check_n_agents(h, who, n_agents, E, A)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    GuideArgs g{};
    if (int rc = upload_walls(h, L, walls, &g.walls, w)) return rc;
    const bool host = mem == JMID_MEM_HOST;
    const size_t M2 = (size_t)E * K * A * T * 2, rows = (size_t)E * K * GDE_COLS;
    g.E = E; g.A = A; g.K = K; g.T = T; g.n_inner = n_inner; g.L = L;
    g.threshold = threshold; g.margin = margin; g.tau = tau; g.weight = weight; g.dt = (double)dt; g.wall_radius = wall_radius;
    if (host) h->last_pos = nullptr;      // (as in jmid_encode)
    Staging st(h, mem, h->kde_ws, who);
    g.x = x_out;
    if (host) st.add(&g.x, x, x_out, M2 * sizeof(float));      // up from x, worked on in place, down to x_out
    st.in(&g.p0, p0, (size_t)E * A * 2);
    if (guide_out) st.out(&g.out, guide_out, rows);
    if (int rc = st.begin()) return rc;
    if (!host && x_out != x) HIPCHK(h, hipMemcpyAsync(x_out, x, M2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (g.out) HIPCHK(h, hipMemsetAsync(g.out, 0, rows * sizeof(float), h->stream));
    if (n_agents) {
        if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
        g.n_agents = h->nag.get<int>();
    }
    if (weight > 0.0) {
        ProfScope ps(h, KC_GUIDE, h->stream);
        HIPCHK(h, launch_guide(g, h->stream));
    }
    return st.end();
}

// jmid_denoise_guided (seeded null) and jmid_denoise_guided_seeded: a DDIM denoise call with the guide kernel behind every step-table entry
// whose weight is > 0; n_agents null, or a padded call.  What is about the table (DDPM, the weights) is refused by check_call
static int guided_entry(jmid_handle_t h, const char* who, int E, int A, int K, int T, const int32_t* n_agents, const float* x_T, const SeedArgs* seeded,
                        const float* ctx, const float* p0, float dt, int precision, double threshold, double margin, double tau,
                        const double* weights, int n_inner, int L, const double* walls, double wall_radius, float* vel_out, float* pos_out,
                        float* guide_out, int mem) {
    if (!h) return JMID_EINVAL;
    const std::string w(who);
    if (int rc = guide_check(h, w, E, A, K, T, p0, dt, threshold, margin, tau, n_inner, wall_radius)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    GuideCall gc;
    gc.threshold = threshold; gc.margin = margin; gc.tau = tau; gc.weights = weights; gc.n_inner = n_inner; gc.L = L;
    gc.wall_radius = wall_radius; gc.guide_out = guide_out;
    if (int rc = upload_walls(h, L, walls, &gc.walls, w)) return rc;
    DenoiseCall c{E, A, K, T, precision, mem};
    c.x_in = x_T; c.seeded = seeded; c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out; c.n_agents = n_agents;
    c.guide = &gc; c.who = who;
    return run_network(h, c);
}

int jmid_denoise_guided(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x_T, const float* ctx, const float* p0,
                        float dt, int precision, double threshold, double margin, double tau, const double* weights, int n_inner, int L,
                        const double* walls, double wall_radius, float* vel_out, float* pos_out, float* guide_out, int mem) {
    if (h && !x_T) return fail(h, JMID_EINVAL, "jmid_denoise_guided: null x_T");
    return guided_entry(h, "jmid_denoise_guided", E, A, K, T, n_agents, x_T, nullptr, ctx, p0, dt, precision, threshold, margin, tau, weights, n_inner,
                        L, walls, wall_radius, vel_out, pos_out, guide_out, mem);
}

int jmid_denoise_guided_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids,
                               const float* ctx, const float* p0, float dt, int precision, double threshold, double margin, double tau,
                               const double* weights, int n_inner, int L, const double* walls, double wall_radius, float* vel_out,
                               float* pos_out, float* guide_out, int mem) {
    const SeedArgs sa{seed, episode_ids};
    return guided_entry(h, "jmid_denoise_guided_seeded", E, A, K, T, n_agents, nullptr, &sa, ctx, p0, dt, precision, threshold, margin, tau, weights,
                        n_inner, L, walls, wall_radius, vel_out, pos_out, guide_out, mem);
}

// jmid_topk (n_agents null) and jmid_topk_padded
static int topk_entry(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* pos, const float* bw, float* sel,
                      float* logw, int mem) {
    if (!h || !sel || !logw || E <= 0 || A <= 0 || K <= 1 || T <= 0) return fail(h, JMID_EINVAL, "bad argument");
    if (k < 1 || k > K) return fail(h, JMID_EINVAL, "k must be in 1..K");
    if (A > 32 || K > 1024 || T > 24) return fail(h, JMID_EINVAL, "jmid_topk supports A <= 32, K <= 1024, T <= 24");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos && !resident_positions(h, E, A, K, T)) return JMID_EINVAL;
    const char* who = n_agents ? "jmid_topk_padded" : "jmid_topk";
    const float *dpos = h->last_pos, *dbw = nullptr;
    float *dsel, *dlw;
    char* ws;
    Staging st(h, mem, h->kde_ws, who);
    st.scratch(&ws, kde_workspace(E, A, K, T, nullptr, nullptr));
    if (bw) st.in(&dbw, bw, (size_t)T, true);      // (bw has always gone through the workspace, in device mode too: the entry enqueues what it did)
    if (pos) st.in(&dpos, pos, (size_t)E * K * A * T * 2);
    st.out(&dsel, sel, (size_t)E * A * k * T * 2);
    st.out(&dlw, logw, (size_t)E * A * k);
    if (int rc = st.begin()) return rc;
    if (n_agents)
        if (int rc = h->nag.upload(h, n_agents, E, who)) return rc;
    if (int rc = topk_on_device(h, who, E, A, K, T, k, dpos, dbw, dsel, dlw, n_agents ? h->nag.get<int>() : nullptr, ws)) return rc;
    return st.end();
}

int jmid_topk(jmid_handle_t h, int E, int A, int K, int T, int k, const float* pos, const float* bw, float* sel, float* logw,
              int mem) {
    return topk_entry(h, E, A, K, T, k, nullptr, pos, bw, sel, logw, mem);
}

int jmid_topk_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* pos, const float* bw, float* sel,
                     float* logw, int mem) {
    if (!h) return JMID_EINVAL;
    if (int rc = check_n_agents(h, "jmid_topk_padded", n_agents, E, A)) return rc;
    return topk_entry(h, E, A, K, T, k, n_agents, pos, bw, sel, logw, mem);
}

// what the chained entries' calls start from: the dimensions, dt, the precision and the entry's name
static ChainCall chain_call(const char* who, int E, int A, int K, int T, int k, float dt, int precision) {
    ChainCall c{E, A, K, T, k, precision};
    c.dt = dt; c.who = who;
    return c;
}

// jmid_predict and jmid_predict_padded: the five inputs are host arrays
static int predict_entry(jmid_handle_t h, const ChainCall& c) {
    if (!h) return JMID_EINVAL;
    if (int rc = check_ready(h)) return rc;
    const std::string w(c.who);
    if (c.E <= 0 || c.A <= 0 || c.K <= 0 || c.T <= 0 || c.k < 1 || c.k > c.K) return fail(h, JMID_EINVAL, w + ": bad dimensions");
    if (!c.x_st || !c.nbr_sum || !c.edge_mask || !c.x_T || !c.p0) return fail(h, JMID_EINVAL, w + ": null input");
    if (c.rank() && (!c.sel || !c.logw)) return fail(h, JMID_EINVAL, w + ": k < K needs sel and logw");
    if (!c.rank() && !c.pos_out) return fail(h, JMID_EINVAL, w + ": k == K needs pos_out");
    if (c.rank() && (c.A > 32 || c.K > 1024 || c.T > 24)) return fail(h, JMID_EINVAL, w + ": the device top-k supports A <= 32, K <= 1024, T <= 24");
    if (h->ddpm) return fail(h, JMID_EINVAL, w + " samples with DDIM (MID.eval_sicnav: sampling=\"ddim\", MID/mid.py:333)");
    HIPCHK(h, hipSetDevice(h->device));
    return predict_chain(h, c);
}

int jmid_predict_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* x_st, const float* nbr_sum,
                        const float* edge_mask, const float* x_T, const float* p0, float dt, int precision, const float* bw, float* sel,
                        float* logw, float* pos_out) {
    if (!h) return JMID_EINVAL;
    if (int rc = check_n_agents(h, "jmid_predict_padded", n_agents, E, A)) return rc;
    ChainCall c = chain_call("jmid_predict_padded", E, A, K, T, k, dt, precision);
    c.padded = true; c.n_agents = n_agents;
    c.x_st = x_st; c.nbr_sum = nbr_sum; c.edge_mask = edge_mask; c.x_T = x_T; c.p0 = p0; c.bw = bw;
    c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_entry(h, c);
}

int jmid_predict(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_st, const float* nbr_sum, const float* edge_mask,
                 const float* x_T, const float* p0, float dt, int precision, const float* bw, float* sel, float* logw, float* pos_out) {
    ChainCall c = chain_call("jmid_predict", E, A, K, T, k, dt, precision);
    c.x_st = x_st; c.nbr_sum = nbr_sum; c.edge_mask = edge_mask; c.x_T = x_T; c.p0 = p0; c.bw = bw;
    c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_entry(h, c);
}

// what the scene builds' calls start from: everything the four entries share but the source
static SceneBuild scene_build(const char* who, int E, int N, int F, double time_step, int horizon, int force_all_in_cluster, int mem) {
    SceneBuild b{who, E, N, F};
    b.time_step = time_step; b.horizon = horizon; b.force_all_in_cluster = force_all_in_cluster; b.mem = mem;
    return b;
}

// the refusal jmid_build_scene_absent and jmid_build_scene_stamped_coast share: an episode whose pedestrians are all -1 (-1: none)
static int episode_with_nobody(const int32_t* first_frame, int E, int N) {
    for (int e = 0; e < E; ++e) {
        int left = 0;
        for (int j = 1; j <= N; ++j) left += first_frame[(size_t)e * (N + 1) + j] >= 0 ? 1 : 0;
        if (!left) return e;
    }
    return -1;
}

// jmid_build_scene, jmid_build_scene_var (first_frame given) and jmid_build_scene_absent (-1 allowed for a pedestrian): every refusal
// comes before the resident scene is touched
static int build_scene_entry(jmid_handle_t h, SceneBuild b) {
    if (!h) return JMID_EINVAL;
    const std::string who(b.who);
    if (b.E <= 0 || !b.human_xy || !b.robot_xy || !b.in_cluster_out || !b.robot_in_cluster_out || !b.n_in_out) return fail(h, JMID_EINVAL, who + ": bad argument");
    if (int rc = check_scene_dims(h, b.who, b.N, b.F, b.cv_out, b.horizon, b.time_step)) return rc;
    if (b.first_frame)
        for (int e = 0; e < b.E; ++e)
            for (int j = 0; j <= b.N; ++j) {
                const int f = b.first_frame[(size_t)e * (b.N + 1) + j];
                if ((f < 0 && !(b.allow_absent && j > 0 && f == -1)) || f > b.F - 1)
                    return fail(h, JMID_EINVAL, who + ": first_frame[" + std::to_string(e) + ", " + std::to_string(j) + "] = " + std::to_string(f) + " is outside 0..F-1");
                if (j == 0 && f > b.F - 2 && !b.force_all_in_cluster)
                    return fail(h, JMID_EINVAL, who + ": the robot of episode " + std::to_string(e) + " has fewer than 2 frames");
            }
    if (b.allow_absent) {
        if (!b.first_frame) return fail(h, JMID_EINVAL, who + ": null first_frame");
        const int e = episode_with_nobody(b.first_frame, b.E, b.N);
        if (e >= 0) return fail(h, JMID_EINVAL, who + ": episode " + std::to_string(e) + " has no pedestrian left (every first_frame is -1)");
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = order_in(h, b.mem)) return rc;
    b.src = b.mem == JMID_MEM_HOST ? SCENE_HOST_ARRAYS : SCENE_DEVICE_ARRAYS;
    if (int rc = build_scene_resident(h, b)) return rc;
    return order_out(h, b.mem);
}

int jmid_build_scene(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, double time_step, int horizon,
                     int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out, int* n_in_out, double* cv_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene", E, N, F, time_step, horizon, force_all_in_cluster, mem);
    b.human_xy = human_xy; b.robot_xy = robot_xy;
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    return build_scene_entry(h, b);
}

int jmid_build_scene_var(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, const int32_t* first_frame,
                         double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out, int* n_in_out,
                         double* cv_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene_var", E, N, F, time_step, horizon, force_all_in_cluster, mem);
    b.human_xy = human_xy; b.robot_xy = robot_xy; b.first_frame = first_frame;
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    return build_scene_entry(h, b);
}

int jmid_build_scene_absent(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, const int32_t* first_frame,
                            double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out,
                            int* n_in_out, double* cv_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene_absent", E, N, F, time_step, horizon, force_all_in_cluster, mem);
    b.human_xy = human_xy; b.robot_xy = robot_xy; b.first_frame = first_frame; b.allow_absent = true;
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    return build_scene_entry(h, b);
}

int jmid_scene_get_first_index(jmid_handle_t h, int32_t* out, int mem) {
    if (!h) return JMID_EINVAL;
    const jmid_ctx::SceneWs& sc = h->scene;
    if (!sc.E) return fail(h, JMID_EINVAL, "jmid_scene_get_first_index needs a preceding jmid_build_scene on this handle");
    if (!out) return fail(h, JMID_EINVAL, "jmid_scene_get_first_index: null output");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = order_in(h, mem)) return rc;
    const size_t bytes = (size_t)sc.E * sc.N * 4;
    const bool host = mem == JMID_MEM_HOST;
    // a scene built without first_frame: every track starts at frame 0
    if (sc.has_first()) {
        HIPCHK(h, hipMemcpyAsync(out, sc.arr.first_index.p, bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    } else if (host) {
        std::memset(out, 0, bytes);
    } else {
        HIPCHK(h, hipMemsetAsync(out, 0, bytes, h->stream));
    }
    if (host) HIPCHK(h, hipStreamSynchronize(h->stream));
    return order_out(h, mem);
}

// the raw frames of jmid_build_scene_stamped / _stamped_var (where the build's `mem` says), and what only those two return
struct StampedFrames {
    bool tracks;                   // false: frames_kernel, a window shorter than hist_len refused.  true: track_frames_kernel, first_frame
                                   // [E, N + 1] read back with n_grid in the one synchronisation and handed to the build
    int R;
    const double *stamps, *human_xy, *robot_xy;
    const int* n_frames;
    int* n_grid_out;
    int32_t* first_frame_out;      // tracks only, or null
    bool coast = false;            // tracks only: track_frames_coast_kernel - a pedestrian who is not seen in the anchor frame is coasted over at
    int max_coast = 0;             // most max_coast bins or left out (first_frame -1, which the build then takes), never refused; coast [E, N]
    int32_t* coast_out = nullptr;  // joins the one download; or null
};

// jmid_build_scene_stamped, jmid_build_scene_stamped_var and jmid_build_scene_stamped_coast: b states everything but the source, which is
// the grid block made here
static int build_scene_stamped_entry(jmid_handle_t h, SceneBuild b, const StampedFrames& s) {
    if (!h) return JMID_EINVAL;
    const std::string who(b.who);
    const int E = b.E, N = b.N, R = s.R, mem = b.mem;
    if (E <= 0 || !s.stamps || !s.human_xy || !s.robot_xy || !b.in_cluster_out || !b.robot_in_cluster_out || !b.n_in_out || !s.n_grid_out)
        return fail(h, JMID_EINVAL, who + ": bad argument");
    if (R < 1 || R > FRM_MAX_R) return fail(h, JMID_EINVAL, who + " supports 1 <= R <= 64 raw frames");
    const int F = b.F = h->hist_len;
    if (int rc = check_scene_dims(h, b.who, N, F, b.cv_out, b.horizon, b.time_step)) return rc;
    if (s.coast && (s.max_coast < 0 || s.max_coast > F - 2))
        return fail(h, JMID_EINVAL, who + ": max_coast = " + std::to_string(s.max_coast) + " is outside 0..F-2");
    // w = round(time_step * 100) as Python rounds it (to nearest, ties to even)
    const double wd = std::nearbyint(b.time_step * 100.0);
    if (!(wd >= 1.0) || wd > 9.0e15) return fail(h, JMID_EINVAL, who + ": round(time_step * 100) must be at least 1");
    const bool host = mem == JMID_MEM_HOST;
    if (host && s.n_frames)
        for (int e = 0; e < E; ++e)
            if (s.n_frames[e] < 1 || s.n_frames[e] > R)
                return fail(h, JMID_EINVAL, who + ": n_frames[" + std::to_string(e) + "] = " + std::to_string(s.n_frames[e]) + " is outside 1..R");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = order_in(h, mem)) return rc;
    const size_t b_st = (size_t)E * R * 8, b_hum = (size_t)E * R * N * 2 * 8, b_rob = (size_t)E * R * 2 * 8, b_nf = s.n_frames ? (size_t)E * 4 : 0;
    // the grid block frames_kernel writes | n_grid (tracks: and first_frame [E, N + 1] behind it, coast: and coast [E, N] behind that, one
    // download) | the staged raw frames (host mode): stamps, human_xy, robot_xy, n_frames
    const size_t n_first = s.tracks ? (size_t)E * (N + 1) : 0, n_coast = s.coast ? (size_t)E * N : 0, b_back = ((size_t)E + n_first + n_coast) * 4;
    const size_t o_ng = grid_block(E, N, F, nullptr, nullptr), o_st = o_ng + align_up(b_back), o_rh = o_st + (host ? align_up(b_st) : 0),
                 o_rr = o_rh + (host ? align_up(b_hum) : 0), o_nf = o_rr + (host ? align_up(b_rob) : 0), need = o_nf + (host ? align_up(b_nf) : 0), raw = need - o_st;
    if (int rc = h->frames_dev.reserve(h, need, b.who)) return rc;
    if (int rc = h->pin.reserve(h, raw + b_back, b.who)) return rc;
    char *const fd = h->frames_dev.p, *const pin = h->pin.p;
    GridBlock gb;
    grid_block(E, N, F, fd, &gb);
    TrackCoastArgs t{};
    FramesArgs& f = t;
    f.E = E; f.N = N; f.R = R; f.F = F;
    f.w = (long long)wd;
    f.stamps = s.stamps; f.human_xy = s.human_xy; f.robot_xy = s.robot_xy; f.n_frames = s.n_frames;
    f.o_human = gb.human_xy; f.o_robot = gb.robot_xy; f.o_pose = gb.pose_now; f.o_n_grid = reinterpret_cast<int*>(fd + o_ng);
    t.o_first = f.o_n_grid + E;
    t.o_coast = t.o_first + n_first; t.max_coast = s.max_coast;
    if (host) {
        std::memcpy(pin, s.stamps, b_st);
        std::memcpy(pin + (o_rh - o_st), s.human_xy, b_hum);
        std::memcpy(pin + (o_rr - o_st), s.robot_xy, b_rob);
        if (s.n_frames) std::memcpy(pin + (o_nf - o_st), s.n_frames, b_nf);
        HIPCHK(h, hipMemcpyAsync(fd + o_st, pin, raw, hipMemcpyHostToDevice, h->stream));
        f.stamps = reinterpret_cast<const double*>(fd + o_st); f.human_xy = reinterpret_cast<const double*>(fd + o_rh);
        f.robot_xy = reinterpret_cast<const double*>(fd + o_rr);
        f.n_frames = s.n_frames ? reinterpret_cast<const int*>(fd + o_nf) : nullptr;
    }
    if (s.coast) HIPCHK(h, launch_track_frames_coast(t, h->stream));
    else if (s.tracks) HIPCHK(h, launch_track_frames(t, h->stream));
    else HIPCHK(h, launch_frames(f, h->stream));
    int* ng = reinterpret_cast<int*>(pin + raw);
    HIPCHK(h, hipMemcpyAsync(ng, f.o_n_grid, b_back, hipMemcpyDeviceToHost, h->stream));
    if (!host) {
        HIPCHK(h, hipMemcpyAsync(s.n_grid_out, f.o_n_grid, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream));
        if (s.first_frame_out) HIPCHK(h, hipMemcpyAsync(s.first_frame_out, t.o_first, n_first * 4, hipMemcpyDeviceToDevice, h->stream));
        if (s.coast_out) HIPCHK(h, hipMemcpyAsync(s.coast_out, t.o_coast, n_coast * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (host) {
        std::memcpy(s.n_grid_out, ng, (size_t)E * 4);
        if (s.first_frame_out) std::memcpy(s.first_frame_out, ng + E, n_first * 4);
        if (s.coast_out) std::memcpy(s.coast_out, ng + E + n_first, n_coast * 4);
    }
    for (int e = 0; e < E; ++e)
        if (ng[e] < 0) {
            (void)order_out(h, mem);
            return fail(h, JMID_EINVAL, who + ": n_frames[" + std::to_string(e) + "] is outside 1..R");
        }
    const int F_min = s.tracks ? 2 : F;                       // a per-track table starts every node where its own frames start
    for (int e = 0; e < E; ++e)
        if (ng[e] < F_min) {
            const int got = ng[e];
            (void)order_out(h, mem);
            return fail(h, JMID_EHISTORY, who + ": episode " + std::to_string(e) + " has " + std::to_string(got) +
                                              " history frames on the time_step grid, " + std::to_string(F_min) + " needed");
        }
    // (build_scene_resident stages through the pinned block again: first_frame leaves it first)
    std::vector<int32_t> first(ng + E, ng + E + n_first);
    if (s.coast) {                                            // a -1 is a pedestrian left out of the scene; somebody has to be left
        const int e = episode_with_nobody(first.data(), E, N);
        if (e >= 0) {
            (void)order_out(h, mem);
            return fail(h, JMID_EINVAL, who + ": episode " + std::to_string(e) + " has no pedestrian left (nobody is seen within max_coast bins of the newest kept frame)");
        }
    }
    for (size_t q = 0; q < n_first && !s.coast; ++q)
        if (first[q] < 0) {
            (void)order_out(h, mem);
            return fail(h, JMID_EINVAL, who + ": episode " + std::to_string(q / (N + 1)) + ", track " + std::to_string((int)(q % (N + 1)) - 1) +
                                            " is not seen in the newest kept frame (leave the track out)");
        }
    b.src = SCENE_DEVICE_GRID;
    b.human_xy = reinterpret_cast<const double*>(fd);
    b.first_frame = s.tracks ? first.data() : nullptr;
    if (int rc = build_scene_resident(h, b)) return rc;
    return order_out(h, mem);
}

int jmid_build_scene_stamped(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                             const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                             uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene_stamped", E, N, 0, time_step, horizon, force_all_in_cluster, mem);
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    return build_scene_stamped_entry(h, b, StampedFrames{false, R, stamps, human_xy, robot_xy, n_frames, n_grid_out, nullptr});
}

int jmid_build_scene_stamped_var(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                                 const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                                 uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int32_t* first_frame_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene_stamped_var", E, N, 0, time_step, horizon, force_all_in_cluster, mem);
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    return build_scene_stamped_entry(h, b, StampedFrames{true, R, stamps, human_xy, robot_xy, n_frames, n_grid_out, first_frame_out});
}

int jmid_build_scene_stamped_coast(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                                   const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                                   uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int32_t* first_frame_out,
                                   int max_coast, int32_t* coast_out, int mem) {
    SceneBuild b = scene_build("jmid_build_scene_stamped_coast", E, N, 0, time_step, horizon, force_all_in_cluster, mem);
    b.in_cluster_out = in_cluster_out; b.robot_in_cluster_out = robot_in_cluster_out; b.n_in_out = n_in_out; b.cv_out = cv_out;
    b.allow_absent = true;
    StampedFrames s{true, R, stamps, human_xy, robot_xy, n_frames, n_grid_out, first_frame_out};
    s.coast = true; s.max_coast = max_coast; s.coast_out = coast_out;
    return build_scene_stamped_entry(h, b, s);
}

int jmid_scene_get_frames(jmid_handle_t h, double* human_xy_out, double* robot_xy_out, double* pose_now_out, int mem) {
    if (!h) return JMID_EINVAL;
    const jmid_ctx::SceneWs& sc = h->scene;
    if (!sc.E) return fail(h, JMID_EINVAL, "jmid_scene_get_frames needs a preceding jmid_build_scene on this handle");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = order_in(h, mem)) return rc;
    const GridBlock& gb = sc.arr.grid;
    const size_t F = h->hist_len, row = (size_t)sc.N * 2 * 8;
    const hipMemcpyKind kind = mem == JMID_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (human_xy_out) HIPCHK(h, hipMemcpyAsync(human_xy_out, gb.human_xy.p, gb.human_xy.bytes(), kind, h->stream));
    if (robot_xy_out) HIPCHK(h, hipMemcpyAsync(robot_xy_out, gb.robot_xy.p, gb.robot_xy.bytes(), kind, h->stream));
    if (pose_now_out) {
        if (sc.stamped) HIPCHK(h, hipMemcpyAsync(pose_now_out, gb.pose_now.p, gb.pose_now.bytes(), kind, h->stream));
        else            // the last frame of every episode's grid
            HIPCHK(h, hipMemcpy2DAsync(pose_now_out, row, gb.human_xy.p + (F - 1) * (size_t)sc.N * 2, F * row, row, sc.E, kind, h->stream));
    }
    if (mem == JMID_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
    return order_out(h, mem);
}

int jmid_scene_get(jmid_handle_t h, float* x, float* x_st, float* nbr_sum, float* edge_mask, float* p0, int mem) {
    if (!h) return JMID_EINVAL;
    const jmid_ctx::SceneWs& sc = h->scene;
    if (!sc.E) return fail(h, JMID_EINVAL, "jmid_scene_get needs a preceding jmid_build_scene on this handle");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = order_in(h, mem)) return rc;
    const SceneArrays& a = sc.arr;
    const hipMemcpyKind kind = mem == JMID_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (x) HIPCHK(h, hipMemcpyAsync(x, a.x.p, a.x.bytes(), kind, h->stream));
    if (x_st) HIPCHK(h, hipMemcpyAsync(x_st, a.x_st.p, a.x_st.bytes(), kind, h->stream));
    if (nbr_sum) HIPCHK(h, hipMemcpyAsync(nbr_sum, a.nbr_sum.p, a.nbr_sum.bytes(), kind, h->stream));
    if (edge_mask) HIPCHK(h, hipMemcpyAsync(edge_mask, a.edge_mask.p, a.edge_mask.bytes(), kind, h->stream));
    if (p0) HIPCHK(h, hipMemcpyAsync(p0, a.p0.p, a.p0.bytes(), kind, h->stream));
    if (mem == JMID_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
    return order_out(h, mem);
}

int jmid_predict_scene(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw, float* sel,
                       float* logw, float* pos_out) {
    ChainCall c = chain_call("jmid_predict_scene", E, A, K, T, k, dt, precision);
    c.x_T = x_T; c.bw = bw; c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_scene_entry(h, c);
}

int jmid_forecast_scene(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                        double* forecasts_out, double* logw_out) {
    ChainCall c = chain_call("jmid_forecast_scene", E, A, K, T, k, dt, precision);
    c.forecast = true; c.x_T = x_T; c.bw = bw; c.forecasts_out = forecasts_out; c.logw_out = logw_out;
    return predict_scene_entry(h, c);
}

int jmid_predict_scene_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt, int precision,
                              const float* bw, float* sel, float* logw, float* pos_out) {
    const SeedArgs sa{seed, episode_ids};
    ChainCall c = chain_call("jmid_predict_scene_seeded", E, A, K, T, k, dt, precision);
    c.seeded = &sa; c.bw = bw; c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_scene_entry(h, c);
}

int jmid_forecast_scene_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt, int precision,
                               const float* bw, double* forecasts_out, double* logw_out) {
    const SeedArgs sa{seed, episode_ids};
    ChainCall c = chain_call("jmid_forecast_scene_seeded", E, A, K, T, k, dt, precision);
    c.forecast = true; c.seeded = &sa; c.bw = bw; c.forecasts_out = forecasts_out; c.logw_out = logw_out;
    return predict_scene_entry(h, c);
}

int jmid_predict_scene_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                              float* sel, float* logw, float* pos_out) {
    ChainCall c = chain_call("jmid_predict_scene_padded", E, A, K, T, k, dt, precision);
    c.padded = true; c.x_T = x_T; c.bw = bw; c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_scene_entry(h, c);
}

int jmid_forecast_scene_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                               double* forecasts_out, double* logw_out) {
    ChainCall c = chain_call("jmid_forecast_scene_padded", E, A, K, T, k, dt, precision);
    c.forecast = c.padded = true; c.x_T = x_T; c.bw = bw; c.forecasts_out = forecasts_out; c.logw_out = logw_out;
    return predict_scene_entry(h, c);
}

int jmid_predict_scene_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                                     int precision, const float* bw, float* sel, float* logw, float* pos_out) {
    const SeedArgs sa{seed, episode_ids};
    ChainCall c = chain_call("jmid_predict_scene_padded_seeded", E, A, K, T, k, dt, precision);
    c.padded = true; c.seeded = &sa; c.bw = bw; c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return predict_scene_entry(h, c);
}

int jmid_forecast_scene_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                                      int precision, const float* bw, double* forecasts_out, double* logw_out) {
    const SeedArgs sa{seed, episode_ids};
    ChainCall c = chain_call("jmid_forecast_scene_padded_seeded", E, A, K, T, k, dt, precision);
    c.forecast = c.padded = true; c.seeded = &sa; c.bw = bw; c.forecasts_out = forecasts_out; c.logw_out = logw_out;
    return predict_scene_entry(h, c);
}

// The constraints value of a constrained chain from the entries' common argument list
static ChainConstraints chain_constraints(double threshold, const double* guide_weights, int n_inner, double guide_margin, double guide_tau,
                                          int guide_walls, int repair, double margin, double tau, double step, int max_iter, int repair_walls, int L,
                                          const double* walls, double wall_radius, float* guide_out, float* sample_out, int32_t* episode_out,
                                          float* wall_out) {
    ChainConstraints k;
    k.threshold = threshold;
    k.guide_weights = guide_weights; k.n_inner = n_inner; k.guide_margin = guide_margin; k.guide_tau = guide_tau; k.guide_walls = guide_walls != 0;
    k.repair = repair != 0; k.margin = margin; k.tau = tau; k.step = step; k.max_iter = max_iter; k.repair_walls = repair_walls != 0;
    k.L = L; k.walls = walls; k.wall_radius = wall_radius;
    k.guide_out = guide_out; k.sample_out = sample_out; k.episode_out = episode_out; k.wall_out = wall_out;
    return k;
}

// What a constrained chain refuses on top of its namesake, before anything is enqueued: what jmid_denoise_guided (guide_check, the weights)
// and jmid_repair_collisions_walls (repair_check) refuse for the same arguments, walls asked for with L = 0, a DDPM table
static int check_constraints(jmid_handle_t h, const ChainCall& c) {
    if (!h) return JMID_EINVAL;
    if (int rc = check_ready(h)) return rc;
    const ChainConstraints& k = *c.cons;
    const std::string w(c.who);
    if (h->ddpm) return fail(h, JMID_EINVAL, w + ": a constrained chain samples with DDIM only (a DDPM table is installed)");
    if (k.L < 0 || k.L > WLS_MAX_L) return fail(h, JMID_EINVAL, w + " supports 0 <= L <= 64 walls");
    if (k.L == 0 && ((k.guided() && k.guide_walls) || (k.repair && k.repair_walls)))
        return fail(h, JMID_EINVAL, w + ": guide_walls / repair_walls need L > 0 walls");
    if (k.walled() && !k.walls) return fail(h, JMID_EINVAL, w + ": null walls with L > 0");
    static const float present = 0.f;      // (a scene chain's p0 is the resident scene's: there is always one)
    const float* p0 = c.scene ? &present : c.p0;
    if (k.guided()) {
        if (int rc = guide_check(h, w, c.E, c.A, c.K, c.T, p0, c.dt, k.threshold, k.guide_margin, k.guide_tau, k.n_inner, k.guide_walls ? k.wall_radius : 0.0))
            return rc;
        for (size_t i = 0; i < h->beta.size(); ++i)
            if (!(k.guide_weights[i] >= 0.0) || !std::isfinite(k.guide_weights[i]))
                return fail(h, JMID_EINVAL, w + ": weights[" + std::to_string(i) + "] must be finite and >= 0");
    }
    if (k.repair) {
        if (c.E <= 0) return fail(h, JMID_EINVAL, w + ": bad argument");
        if (int rc = repair_check(h, w, k.repair_walls, c.E, c.A, c.K, c.T, true, c.dt, k.threshold, k.margin, k.tau, k.step, k.max_iter, k.wall_radius)) return rc;
    }
    if (!k.guided() && !k.repair && (!(k.threshold >= 0.0) || !std::isfinite(k.threshold)))
        return fail(h, JMID_EINVAL, w + ": the threshold must be finite and >= 0");
    if (k.walled())
        for (int i = 0; i < k.L * 4; ++i)
            if (!std::isfinite(k.walls[i])) return fail(h, JMID_EINVAL, w + ": a wall has a non-finite coordinate");
    return 0;
}

int jmid_predict_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* x_st, const float* nbr_sum,
                             const float* edge_mask, const float* x_T, const float* p0, float dt, int precision, const float* bw, double threshold,
                             const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                             double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                             double wall_radius, float* sel, float* logw, float* pos_out, float* guide_out, float* sample_out,
                             int32_t* episode_out, float* wall_out) {
    if (!h) return JMID_EINVAL;
    const ChainConstraints cons = chain_constraints(threshold, guide_weights, n_inner, guide_margin, guide_tau, guide_walls, repair, margin, tau, step,
                                                    max_iter, repair_walls, L, walls, wall_radius, guide_out, sample_out, episode_out, wall_out);
    ChainCall c = chain_call("jmid_predict_constrained", E, A, K, T, k, dt, precision);
    if (n_agents) {
        if (int rc = check_n_agents(h, c.who, n_agents, E, A)) return rc;
        c.padded = true; c.n_agents = n_agents;
    }
    c.x_st = x_st; c.nbr_sum = nbr_sum; c.edge_mask = edge_mask; c.x_T = x_T; c.p0 = p0; c.bw = bw;
    c.sel = sel; c.logw = logw; c.pos_out = pos_out; c.cons = &cons;
    if (int rc = check_constraints(h, c)) return rc;
    return predict_entry(h, c);
}

// jmid_predict_scene_constrained and jmid_forecast_scene_constrained: the scene chain of (padded, x_T or seed) with the constraints value
static int scene_constrained_entry(jmid_handle_t h, ChainCall c, int padded, const float* x_T, uint64_t seed, const uint32_t* episode_ids,
                                   const ChainConstraints& cons) {
    if (!h) return JMID_EINVAL;
    const SeedArgs sa{seed, episode_ids};
    c.padded = padded != 0; c.x_T = x_T; c.cons = &cons;
    if (!x_T) c.seeded = &sa;
    c.scene = true;      // (predict_scene_entry says so too: the check below reads it)
    if (int rc = check_constraints(h, c)) return rc;
    return predict_scene_entry(h, c);
}

int jmid_predict_scene_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, int padded, const float* x_T, uint64_t seed,
                                   const uint32_t* episode_ids, float dt, int precision, const float* bw, double threshold,
                                   const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                                   double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                                   double wall_radius, float* sel, float* logw, float* pos_out, float* guide_out, float* sample_out,
                                   int32_t* episode_out, float* wall_out) {
    const ChainConstraints cons = chain_constraints(threshold, guide_weights, n_inner, guide_margin, guide_tau, guide_walls, repair, margin, tau, step,
                                                    max_iter, repair_walls, L, walls, wall_radius, guide_out, sample_out, episode_out, wall_out);
    ChainCall c = chain_call("jmid_predict_scene_constrained", E, A, K, T, k, dt, precision);
    c.bw = bw; c.sel = sel; c.logw = logw; c.pos_out = pos_out;
    return scene_constrained_entry(h, c, padded, x_T, seed, episode_ids, cons);
}

int jmid_forecast_scene_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, int padded, const float* x_T, uint64_t seed,
                                    const uint32_t* episode_ids, float dt, int precision, const float* bw, double threshold,
                                    const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                                    double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                                    double wall_radius, double* forecasts_out, double* logw_out, float* guide_out, float* sample_out,
                                    int32_t* episode_out, float* wall_out) {
    const ChainConstraints cons = chain_constraints(threshold, guide_weights, n_inner, guide_margin, guide_tau, guide_walls, repair, margin, tau, step,
                                                    max_iter, repair_walls, L, walls, wall_radius, guide_out, sample_out, episode_out, wall_out);
    ChainCall c = chain_call("jmid_forecast_scene_constrained", E, A, K, T, k, dt, precision);
    c.forecast = true; c.bw = bw; c.forecasts_out = forecasts_out; c.logw_out = logw_out;
    return scene_constrained_entry(h, c, padded, x_T, seed, episode_ids, cons);
}

int jmid_denoise_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids,
                               const float* ctx, const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!n_agents) return fail(h, JMID_EINVAL, "jmid_denoise_padded_seeded: null n_agents");
    if (!episode_ids) return fail(h, JMID_EINVAL, "jmid_denoise_padded_seeded: null episode_ids");
    const SeedArgs sa{seed, episode_ids};
    DenoiseCall c{E, A, K, T, precision, mem};
    c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out; c.n_agents = n_agents; c.seeded = &sa;
    c.who = "jmid_denoise_padded_seeded";
    return run_network(h, c);
}

int jmid_noise_fill_padded(jmid_handle_t h, uint64_t seed, int E, int A, int K, int T, const int32_t* n_agents, const uint32_t* episode_ids, int draw,
                           float* out, int mem) {
    return noise_padded_entry(h, seed, E, A, K, T, n_agents, episode_ids, draw, out, mem);
}

int jmid_denoise_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, const float* ctx, const float* p0,
                        float dt, int precision, float* vel_out, float* pos_out, int mem) {
    if (!h) return JMID_EINVAL;
    if (!episode_ids) return fail(h, JMID_EINVAL, "jmid_denoise_seeded: null episode_ids");
    const SeedArgs sa{seed, episode_ids};
    DenoiseCall c{E, A, K, T, precision, mem};
    c.ctx = ctx; c.p0 = p0; c.dt = dt; c.vel_out = vel_out; c.pos_out = pos_out; c.seeded = &sa; c.who = "jmid_denoise_seeded";
    return run_network(h, c);
}

// jmid_denoise_reject_seeded (L = 0, walls and cause_out null), jmid_denoise_reject_walls_seeded and jmid_denoise_reject_padded_seeded
// (padded: n_agents a HOST array [E]): the argument checks, then the loop
static int reject_entry(jmid_handle_t h, const char* who, int E, int A, int K, int T, bool padded, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids, int draw0,
                        const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds, int L, const double* walls,
                        double radius, float* vel_out, float* pos_out, int32_t* slot_out, int32_t* episode_out, int32_t* cause_out, int mem) {
    if (!h) return JMID_EINVAL;
    const std::string w(who);
    if (int rc = check_ready(h)) return rc;
    if (h->ddpm) return fail(h, JMID_EINVAL, w + " samples with DDIM: under a DDPM table the draws 1.. are the steps' z");
    if (E < 1 || K < 1 || K > REJ_MAX_K || T < 2 || T > CLS_MAX_T || A < 1 || A > CLS_MAX_A)
        return fail(h, JMID_EINVAL, w + " supports E >= 1, 1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64");
    if ((size_t)E * K > (size_t)0x7fffffff) return fail(h, JMID_EINVAL, w + ": E * K exceeds the launch grid");
    if (!episode_ids || !ctx) return fail(h, JMID_EINVAL, w + ": null episode_ids or ctx");
    if (!p0) return fail(h, JMID_EINVAL, w + ": null p0 (the predicate is defined on positions)");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(h, JMID_EINVAL, w + ": the threshold must be finite and >= 0");
    if (max_rounds < 0 || max_rounds > 64) return fail(h, JMID_EINVAL, w + ": max_rounds must be in 0..64");
    if (draw0 < 0 || draw0 > 0x7fffffff - 64) return fail(h, JMID_EINVAL, w + ": draw0 must be at least 0 (and draw0 + max_rounds must fit an int)");
    CallMode mode;
    if (!call_mode(precision, &mode)) return fail(h, JMID_EINVAL, w + ": precision must be JMID_PREC_F32, JMID_PREC_F16X3, JMID_PREC_F16X2 or JMID_PREC_F16MX");
    if (mem != JMID_MEM_HOST && mem != JMID_MEM_DEVICE) return fail(h, JMID_EINVAL, w + ": bad mem");
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(h, JMID_EINVAL, w + ": the radius must be finite and >= 0");
    if (padded) {
        if (int rc = check_n_agents(h, who, n_agents, E, A)) return rc;
        if (h->net_kind == JMID_NET_JMID && mode.split && !attn_masked_built(plan_attn(h->d / h->nhead, h->tune), mode.x2 != 0))
            return fail(h, JMID_EINVAL, w + ": a padded call needs the default attention kernel (the attention A/B knobs have no masked form)");
    }
    HIPCHK(h, hipSetDevice(h->device));
    RejectWalls rw;
    rw.L = L; rw.radius = radius;
    if (int rc = upload_walls(h, L, walls, &rw.dev, w)) return rc;
    return reject_loop(h, who, E, A, K, T, n_agents, seed, episode_ids, draw0, ctx, p0, dt, precision, threshold, max_rounds, rw, vel_out, pos_out, slot_out,
                       episode_out, cause_out, mem);
}

int jmid_denoise_reject_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, int draw0, const float* ctx,
                               const float* p0, float dt, int precision, double threshold, int max_rounds, float* vel_out, float* pos_out,
                               int32_t* slot_out, int32_t* episode_out, int mem) {
    return reject_entry(h, "jmid_denoise_reject_seeded", E, A, K, T, false, nullptr, seed, episode_ids, draw0, ctx, p0, dt, precision, threshold, max_rounds, 0,
                        nullptr, 0.0, vel_out, pos_out, slot_out, episode_out, nullptr, mem);
}

int jmid_denoise_reject_walls_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, int draw0,
                                     const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds, int L,
                                     const double* walls, double radius, float* vel_out, float* pos_out, int32_t* slot_out, int32_t* episode_out,
                                     int32_t* cause_out, int mem) {
    return reject_entry(h, "jmid_denoise_reject_walls_seeded", E, A, K, T, false, nullptr, seed, episode_ids, draw0, ctx, p0, dt, precision, threshold,
                        max_rounds, L, walls, radius, vel_out, pos_out, slot_out, episode_out, cause_out, mem);
}

int jmid_denoise_reject_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids,
                                      int draw0, const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds, int L,
                                      const double* walls, double radius, float* vel_out, float* pos_out, int32_t* slot_out, int32_t* episode_out,
                                      int32_t* cause_out, int mem) {
    return reject_entry(h, "jmid_denoise_reject_padded_seeded", E, A, K, T, true, n_agents, seed, episode_ids, draw0, ctx, p0, dt, precision,
                        threshold, max_rounds, L, walls, radius, vel_out, pos_out, slot_out, episode_out, cause_out, mem);
}

int jmid_noise_fill(jmid_handle_t h, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, float* out, int mem) {
    return noise_entry(h, "jmid_noise_fill", seed, E, rows, T, episode_ids, draw, out, nullptr, mem);
}

int jmid_set_chunk_episodes(jmid_handle_t h, int episodes) {
    if (!h || episodes < 0) return JMID_EINVAL;
    h->chunk_eps = episodes;
    drop_graphs(h);
    return JMID_OK;
}

int jmid_set_tuning(jmid_handle_t h, const char* key, int value) {
    if (!h || !key) return JMID_EINVAL;
    const std::string k(key);
    struct Knob {
        const char* name;
        int Tuning::*field;
        int lo, hi;
    };
    // every knob belongs to the handle (h->tune); none is process-wide
#ifdef JMID_DIAGNOSTICS
    static const Knob knobs[] = {
        {"gemm_h_variant", &Tuning::gemm_h_variant, 0, 8},     // 0 auto, 1..8 force a tile variant of the split GEMM
        {"attn_pack", &Tuning::attn_pack, 0, 1},               // 0: one short sequence per wave, 1: packed (iMID)
        {"fuse_embed", &Tuning::fuse_embed, 0, 1},             // 0: separate embed_kernel at the start of every step
        {"bystander_lds", &Tuning::bystander_lds, 0, 160 * 1024},   // unused dynamic LDS requested by row-wise kernels
        {"ln_rows", &Tuning::ln_rows, 0, 128},                 // row tile of the fused GEMM + LayerNorm: 0 auto, 64, 128
        {"ln_fuse", &Tuning::ln_fuse, 0, 2},                   // 0 auto (M >= 7168 tokens), 1 always, 2 never
        {"no_vt_direct", &Tuning::no_vt_direct, 0, 1},         // 1: always V row-major + v_transpose_kernel
        {"gemm_ng", &Tuning::gemm_ng, 0, 64},                  // N-tiles per L2 group of the 256x128 GEMM (0 = auto)
        {"attn_h_variant", &Tuning::attn_h_variant, 0, 2},
        {"vt_stage", &Tuning::vt_stage, 0, 3},                 // V^T of the 256x256 QKV kernel through LDS: 0 / 1 on, 2 off
        {"graph", &Tuning::graph, 0, 2},                       // captured denoise loop of one-chunk calls: 1 on, 0 / 2 off
        {"attn_nsplit", &Tuning::attn_nsplit, 0, 16},
        {"attn_mx", &Tuning::attn_mx, 0, 3},
        {"out_traj", &Tuning::out_traj, 0, 2},
        {"attn_pf", &Tuning::attn_pf, 0, 2},
        {"attn_one_wg", &Tuning::attn_one_wg, 0, 1},
        {"attn_sm", &Tuning::attn_sm, 0, 2},
        {"attn_prio", &Tuning::attn_prio, 0, 2},
        {"mx_ln", &Tuning::mx_ln, 0, 2},
        {"csl_swap", &Tuning::csl_swap, 0, 3},
        {"h1_stage", &Tuning::h1_stage, 0, 2},
        {"gemm_small", &Tuning::gemm_small, 0, 2},             // 1: no deep-ring small-launch GEMM (the round-3 64 x 64 / 128 x 128 shapes)
        {"gemm_pn", &Tuning::gemm_pn, 0, 8},
        {"small_lanes", &Tuning::small_lanes, 0, 2},
        {"small_cmb", &Tuning::small_cmb, 0, 2},               // 2: attn_combine_kernel instead of the split-KV merge inside the out-projection's one-launch GEMM + LayerNorm
        {"small_lnx", &Tuning::small_lnx, 0, 2},               // the one-launch GEMM + LayerNorm with the statistics exchange: 0 on, 2 off (GEMM + add_ln2)
        {"cus", &Tuning::cus, 0, 4096},                         // compute units OUT_LNX may count on (0 = ask the device again, as jmid_create did)
        {"lnx_polls", &Tuning::lnx_polls, 0, 1 << 20},
        {"lnx_withhold", &Tuning::lnx_withhold, 0, 1},
        {"small_lnx2", &Tuning::small_lnx2, 0, 2},             // the same at 33 ... 64 row tiles, two workgroups per CU: 0 on, 2 off
        {"small_qk", &Tuning::small_qk, 0, 2},
        {"small_pn", &Tuning::small_pn, 0, 8},                 // column groups of its XCD tile order: 0 auto
        {"qkv0", &Tuning::qkv0, 0, 2},                         // layer 0's Q / K / V^T: 0 expanded from coefficient tables (qkv0.hpp), 1 the in_proj GEMM, 2 expanded with the table GEMM as one running sum (A/B of the per-tile sums)
        {"tail_fold", &Tuning::tail_fold, 0, 2},               // the step's tail: 0 one 2 x d map per (row, step) (tail_fold.hpp), 1 concat3 / concat4 GEMMs + out_ddim, 2 folded with the one-step table rebuilt every step
#ifdef JMID_ABLATIONS
        {"attn_abl", &Tuning::attn_abl, 0, 1 << 30},           // timing ablations: results are WRONG (tools/attn_abl.py)
        {"gemm_abl", &Tuning::gemm_abl, 0, 1 << 30},
#endif
    };
#endif
    if (k == "lanes") {     // chunks of the denoise loop in flight at once: 1..4
        if (value < 1 || value > jmid_ctx::kMaxLanes) return fail(h, JMID_EINVAL, "lanes must be 1..4");
        h->lanes = value;
        return JMID_OK;
    }
#ifdef JMID_DIAGNOSTICS
    for (const Knob& kn : knobs)
        if (k == kn.name) {
            if (value < kn.lo || value > kn.hi || (k == "ln_rows" && value != 0 && value != 64 && value != 128))
                return fail(h, JMID_EINVAL, k + " out of range");
            h->tune.*(kn.field) = value;
            if (k == "cus" && value == 0) {
                int cus = 0;
                h->tune.cus = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0 ? cus : 256;
            }
            drop_graphs(h);          // captured loops hold the kernel variants the old knobs selected
            return JMID_OK;
        }
#endif
    return fail(h, JMID_EINVAL, "unknown tuning key " + k);
}

int64_t jmid_graph_replays(jmid_handle_t h) { return h ? h->graph_replays : -1; }

int64_t jmid_erange_count(jmid_handle_t h) { return h ? h->erange_calls : -1; }
int64_t jmid_timeout_count(jmid_handle_t h) { return h ? h->lnx_timeouts : -1; }

int jmid_set_caller_stream(jmid_handle_t h, void* stream) {
    if (!h) return JMID_EINVAL;
    h->caller_stream = reinterpret_cast<hipStream_t>(stream);
    return JMID_OK;
}

int jmid_synchronize(jmid_handle_t h) {
    if (!h) return JMID_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return JMID_OK;
}

}  // extern "C"


// libjmid_hip.so -- chunk plan, step workspace, one net evaluation, the denoise loop.
#include "jmid_ctx.hpp"
#include "jmid_launch.hpp"

namespace jmid_host {

void drop_graphs(jmid_ctx* h) {
    for (auto& kv : h->graphs)
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
    h->graphs.clear();
}

// Error paths and arena owners: nothing may still run on a lane stream when the arena is reused or freed.
void sync_lanes(jmid_ctx* h) {
    for (int l = 0; l + 1 < jmid_ctx::kMaxLanes; ++l)
        if (h->lane_stream[l]) (void)hipStreamSynchronize(h->lane_stream[l]);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
}

int ensure_arena(jmid_ctx* h, size_t bytes, const char* who) {
    if (bytes <= h->arena.bytes) return 0;
    drop_graphs(h);
    h->last_pos = nullptr;
    sync_lanes(h);
    return h->arena.reserve(h, bytes, who);
}

struct StepBuffers {
    float *X, *QKV, *ATT, *Y, *H1, *Y3, *Y4;
    // F16X3 path: hi/lo planes
    half_t *Xh, *Xl, *Qh, *Ql, *Kh, *Kl, *Vh, *Vl, *Vth, *Vtl, *Ah, *Al, *H1h, *H1l, *Y3h, *Y3l;
    size_t vt_elems;
    float *Opart, *MLpart;
    float *coef, *uvc;             // layer 0's coefficient rows [steps, Ec A, 3, d] and their image under in_proj [steps, Ec A, 3, 3 d] (qkv0.hpp), or null
    float *weff, *beff;            // the folded tail's maps [steps, Ec A, 2, d] and [steps, Ec A, 2] (tail_fold.hpp), or null
    unsigned long long* ln_xchg;   // exchange granules of the small-launch GEMM + LayerNorm (gemm_small.hpp, OUT_LNX): kLnxWords words, zeroed once per call
};

// One chunk in flight: its step workspace, the stream its steps are enqueued on (lane 0: the handle's own) and, in a seeded DDPM call,
// the z of its one current step.  A value of the call (CallPlan): the handle's stream is never reassigned.
struct Lane : StepBuffers {
    hipStream_t stream;
    float* z;
};

half_t* take_half(Carver& c, size_t n) { return reinterpret_cast<half_t*>(c.take((n + 1) / 2)); }

// attention geometry of a chunk
struct SeqGeom {
    int nseq, S, Spad;
};
SeqGeom seq_geom(const jmid_ctx* h, int Ec, int A, int K, int T) {
    SeqGeom g;
    g.nseq = h->net_kind == JMID_NET_JMID ? Ec : Ec * K * A;
    g.S = h->net_kind == JMID_NET_JMID ? K * A * T : T;
    g.Spad = vt_spad(g.S);
    return g;
}

// qkv0_rows: coefficient rows of layer 0's table (steps x Ec A x 3), 0 = that layer runs its in_proj GEMM
// tail_rows: maps of the folded tail's table (steps x Ec A), 0 = the tail runs its GEMMs: only then are Y3 / Y4 reserved
size_t step_ws_floats(const jmid_ctx* h, size_t Mc, const CallMode& m, const SeqGeom& sg, int nsplit, StepBuffers* sb,
                      char* base, size_t qkv0_rows, size_t tail_rows) {
    Carver c(base);
    StepBuffers s{};
    s.X = c.take(Mc * h->d);
    s.Y = c.take((Mc + 63) / 64 * 64 * h->d);     // (whole 64-row tiles)
    s.ln_xchg = reinterpret_cast<unsigned long long*>(c.take(kLnxWords));
    if (!tail_rows) s.Y4 = c.take(Mc * h->dlow);
    if (!m.split) {
        s.QKV = c.take(Mc * 3 * h->d);
        s.ATT = c.take(Mc * h->d);
        s.H1 = c.take(Mc * h->ff);
        s.Y3 = c.take(Mc * h->dmid);
    } else {
        s.Xh = take_half(c, blk_plane_elems(Mc, h->d));
        s.Xl = take_half(c, blk_plane_elems(Mc, h->d));
        if (h->net_kind == JMID_NET_JMID) {
            s.Qh = take_half(c, Mc * h->d);
            s.Ql = take_half(c, Mc * h->d);
            s.Kh = take_half(c, Mc * h->d);
            s.Kl = take_half(c, Mc * h->d);
            s.Vh = take_half(c, Mc * h->d);
            s.Vl = take_half(c, Mc * h->d);
            s.vt_elems = (size_t)sg.nseq * h->d * sg.Spad;
            s.Vth = take_half(c, s.vt_elems);
            s.Vtl = take_half(c, s.vt_elems);
            if (nsplit > 1) {      // split-KV factor of the attention launch (1 = off)
                s.Opart = c.take((size_t)nsplit * Mc * h->d);
                s.MLpart = c.take((size_t)nsplit * Mc * h->nhead * 2);
            }
            if (qkv0_rows) {
                s.coef = c.take(qkv0_rows * h->d);
                s.uvc = c.take(qkv0_rows * 3 * h->d);
            }
        } else {
            s.QKV = c.take(Mc * 3 * h->d);  // iMID: sequences of T tokens, exact-fp32 attention kernel
        }
        s.Ah = take_half(c, blk_plane_elems(Mc, h->d));
        s.Al = take_half(c, blk_plane_elems(Mc, h->d));
        s.H1h = take_half(c, blk_plane_elems(Mc, h->ff));
        s.H1l = take_half(c, blk_plane_elems(Mc, h->ff));
        if (tail_rows) {
            s.weff = c.take(tail_rows * 2 * h->d);
            s.beff = c.take(tail_rows * 2);
        } else {
            s.Y3h = take_half(c, blk_plane_elems(Mc, h->dmid));
            s.Y3l = take_half(c, blk_plane_elems(Mc, h->dmid));
        }
    }
    if (sb) *sb = s;
    return c.off;
}

// JMID_PREC_F16MX at d_model 512: second-generation LayerNorm kernels (gemm_ln2_mx.hpp) - the lo plane of the residual stream
// is a byte plane (it lives in the memory of the fp16 one), the row statistics are summed in that file's order
bool byte_lo_plane(const jmid_ctx* h, const CallMode& m) { return m.mx && h->d == GLN_BN && h->tune.mx_ln != 2; }

// A residual block of a layer in the split-fp16 modes - X <- LayerNorm(X + A . W^T + bias): out_proj + norm1 (K = d_model) and
// linear2 + norm2 (K = d_ff) - runs in one of four ways.  All four give bit-identical rows.
enum ResidualPath {
    RB_GEMM_LN2,        // row-tile GEMM with the LayerNorm inside, second generation (gemm_ln2_mx.hpp)
    RB_GEMM_LN,         // ... first generation (gemm_ln_f16x3.hpp)
    RB_LNX_SMALL,       // ONE small launch whose workgroups exchange the row statistics (gemm_small.hpp, OUT_LNX)
    RB_GEMM_ADD_LN,     // GEMM -> fp32 Y, then add_ln
};
struct ResidualPlan {
    ResidualPath path;
    int ln_rows;        // RB_GEMM_LN2 / RB_GEMM_LN: the row tile (launch_plan.hpp::plan_ln_rows)
    GemmPlan gemm;      // RB_LNX_SMALL / RB_GEMM_ADD_LN: the GEMM launch
    bool merge;         // RB_LNX_SMALL of out_proj: the split-KV merge of the attention launch rides in front of its K loop (plan_step)
};

// THE function that picks the path of a residual block of M rows; everything else (the step plan, the chunk plan) asks it.
ResidualPlan residual_path(const jmid_ctx* h, const CallMode& m, int M, int K, const CallFacts& cf) {
    // row-complete GEMM with residual + LayerNorm fused in from 7168 tokens (6 episodes
    // per launch: 36.8 vs 39.1 ms per 12-episode call; 5: 33.8 vs 33.5, 4: 29.6 vs 28.8)
    // (enough row tiles to occupy the chip); otherwise GEMM -> fp32 Y -> add_ln
    const Tuning& t = h->tune;
    if (h->d == GLN_BN && t.ln_fuse != 2 && (t.ln_fuse == 1 || M >= 7168))
        return {byte_lo_plane(h, m) ? RB_GEMM_LN2 : RB_GEMM_LN, plan_ln_rows(byte_lo_plane(h, m), M, t), {}, false};
    // one scene in F16MX (one chunk of <= 2048 rows, or two scenes' worth with two workgroups per CU; byte lo plane): GEMM + residual +
    // LayerNorm in ONE small launch (two launches per layer fewer); a handle on which such a kernel ever gave up waiting (lnx_off)
    // stays on the pair
    if (byte_lo_plane(h, m) && !h->lnx_off) {
        const GemmPlan lnx = plan_gemm(GM_MX, EPI_BIAS, OUT_LNX, M, h->d, K, cf, t);
        if (lnx.shape != GS_NONE) return {RB_LNX_SMALL, 0, lnx, false};
    }
    return {RB_GEMM_ADD_LN, 0, plan_gemm(m.gemm, EPI_BIAS, OUT_F32, M, h->d, K, cf, t), false};
}

// Is a batch of `tokens` tokens ONE launch by default (plan_chunks keeps it one chunk)?  Shape and mode (its argument) only.  There are two
// predicates on purpose: this one sizes the split-KV factor, which decides the order in which a sequence's keys are summed, so it
// must not see a knob or lnx_off (the bits of a call must not depend on one); residual_path may, its paths give the same bits.
bool one_launch_shape(const jmid_ctx* h, const CallMode& m, long tokens) { return m.mx && h->d == GLN_BN && tokens <= 2560; }

// Everything one net evaluation on a chunk of Ec episodes decides, decided once per call and chunk size (run_network): the knobs
// and lnx_off cannot change while a call runs.  net_step executes it.
struct StepPlan {
    int Ec, M, T;                // episodes and tokens (Ec * K * A * T) of the chunk, tokens per trajectory
    int R;                       // (episode, agent) rows of the chunk: Ec * A
    bool qkv0;                   // layer 0's Q / K / V^T planes are expanded from coefficient tables (qkv0.hpp) instead of its in_proj GEMM:
                                 // mode and net only, never the token count; the steps a table holds: cf.qkv0_steps
    bool tail_fold;              // concat3 -> concat4 -> output layer as one 2 x d map per (row, step) (tail_fold.hpp): mode and net only (cf.tail_steps)
    CallMode mode;               // of the call: split-fp16 or not, x2, mx, the GEMM mode
    bool mxv2, joint;            // from it: byte lo plane of the residual stream (byte_lo_plane); JMID (joint attention over an episode)
    RowMap rm;
    SeqGeom sg;
    int hd;
    float att_scale;
    bool vt_direct;              // the QKV epilogue writes V^T itself; otherwise V row-major + v_transpose_kernel
    bool k8, q8l;                // bf8 images of K_hi / K_lo, and of Q_lo, written by the QKV epilogue for the attention kernel
    CallFacts cf;                // (the split-KV factor)
    GemmPlan in_proj, linear1, concat3, concat4;      // the GEMM launches of a step in the split-fp16 modes (launch_plan.hpp)
    ResidualPlan out_proj, linear2;
    AttnPlan attn;
    int out_tpw;                 // output kernel: tokens per wave of the per-trajectory form, 0 = one wave per token
    // The time part of the hyper nets the kernels of step i add to every row's hyp: row i of the handle's step table - or, in a loss call,
    // whose rows carry their own timestep inside hyp (loss.hpp), the handle's zeroed row for every step (stride 0).  A value of the call.
    const float* thyp_base;
    size_t thyp_stride;
    const float* thyp(int step) const { return thyp_base + (size_t)step * thyp_stride; }
    // ... and, where such a call's tail is not the folded one, the time part of the output layer's bias per row (OutArgs::tbo) for the
    // chunk whose hyper rows are hyp_chunk: loss_tbo [E A, 2] runs parallel to the call's hyper rows loss_hyp [E A, hl.total]
    const float *loss_hyp, *loss_tbo;
    const float* tbo(const float* hyp_chunk) const { return loss_tbo ? loss_tbo + (size_t)(hyp_chunk - loss_hyp) / thyp_ld * 2 : nullptr; }
    size_t thyp_ld;              // hl.total
};

StepPlan plan_step(const jmid_ctx* h, int Ec, int A, int K, int T, const CallMode& mode, const CallFacts& cf, bool masked = false) {
    StepPlan p{};
    const int d = h->d;
    p.Ec = Ec;
    p.M = Ec * K * A * T;
    p.T = T;
    p.R = Ec * A;
    p.mode = mode;
    const bool split = mode.split;
    p.mxv2 = split && byte_lo_plane(h, mode);
    p.joint = h->net_kind == JMID_NET_JMID;
    p.rm = make_rowmap(T, A, K * A, (unsigned long long)p.M);
    p.sg = seq_geom(h, Ec, A, K, T);
    p.hd = d / h->nhead;
    p.att_scale = 1.0f / sqrtf((float)p.hd);
    p.cf = cf;
    p.thyp_base = h->thyp;
    p.thyp_stride = p.thyp_ld = (size_t)h->hl.total;
    const Tuning& t = h->tune;
    p.attn = plan_attn(p.hd, t);
    p.attn.masked = masked && p.joint;      // (iMID: its rows are independent sequences, nothing to mask)
    p.qkv0 = split && p.joint && t.qkv0 != 1 && d % 32 == 0;      // (d % 32: the K tiles of the table's GEMM - as every GEMM of the net)
    p.tail_fold = split && t.tail_fold != 1 && d % 8 == 0 && d <= kTailMaxD && h->dmid <= kTailMaxMid && h->dlow <= kTailMaxLow;
    if (split) {
        const auto gemm = [&](int epi, int out, int N, int K) { return plan_gemm(mode.gemm, epi, out, p.M, N, K, cf, t); };
        p.in_proj = gemm(EPI_BIAS, p.joint ? OUT_QKV : OUT_F32, 3 * d, d);
        p.linear1 = gemm(EPI_BIAS_RELU, OUT_SPLIT, h->ff, d);
        p.concat3 = gemm(EPI_CSL, OUT_SPLIT, h->dmid, d);
        p.concat4 = gemm(EPI_CSL, OUT_F32, h->dlow, h->dmid);
        p.out_proj = residual_path(h, mode, p.M, d, cf);
        p.linear2 = residual_path(h, mode, p.M, h->ff, cf);
    }
    if (split && p.joint) {
        // S % 4 == 0: the QKV epilogue writes V^T itself; otherwise V row-major + v_transpose_kernel
        p.vt_direct = (p.sg.S % 4 == 0) && !t.no_vt_direct;
        // JMID_PREC_F16MX, head_dim 128 (the LDS-DMA attention kernel): bf8 images of K_hi / K_lo in the K_lo plane's memory, for
        // the logits' correction terms as bf8 MFMAs (attention 7 % faster; "attn_mx" = 2: fp16 terms as in F16X2)
        // (in_proj planned for F16X2's kernels - the register-staged variants a knob can force -: no image stores)
        p.k8 = p.in_proj.mode == GM_MX && p.hd == 128 && t.attn_h_variant == 0 && t.attn_mx != 2;
        p.q8l = p.k8 && t.attn_mx != 3;      // 3: Q_lo as fp16 (A/B)
        // one scene: the partial outputs of a split-KV attention launch are merged in front of the out-projection's K loop
        // (gemm_small.hpp, lnx_combine) when that launch is the one with the LayerNorm inside
        p.out_proj.merge = p.out_proj.path == RB_LNX_SMALL && small_cmb_fits(p.attn, p.cf.attn_nsplit, mode.x2, t);
    }
    if (d <= 512 && p.M % T == 0 && t.out_traj != 2 && (t.out_traj == 1 || p.M >= 4096 * 4)) {
        // one wave per trajectory (T tokens) - or per piece of one, the largest divisor of T that still leaves >= 4096 waves -
        // once there are enough tokens to fill the chip that way: one scene (100 trajectories) takes 14.0 instead of
        // 12.7 ms per call with whole trajectories, a 51-episode chunk 150.3 instead of 151.2
        p.out_tpw = T;
        while (p.out_tpw > 1 && (p.M / p.out_tpw < 4096 || T % p.out_tpw != 0)) --p.out_tpw;
        if (t.out_traj == 1) p.out_tpw = T;
    }
    return p;
}

// One residual block on the path the plan holds for it.  A planes [M, K]: the attention output (out_proj) or linear1's (linear2).
// no_lo_out: the residual stream ends here (norm2 of the last layer: concat3 reads X_hi only), its lo plane is not written
// where it is the byte plane or the mode is F16X2.
int residual_block(jmid_ctx* h, const StepPlan& p, const ResidualPlan& rp, const Lane& ln, const half_t* Ahi, const half_t* Alo,
                   int K, const LinearW& lin, const NormW& nrm, int cls, bool no_lo_out) {
    const int M = p.M, d = h->d;
    unsigned char* Xl8 = p.mxv2 ? reinterpret_cast<unsigned char*>(ln.Xl) : nullptr;
    if (rp.path == RB_GEMM_LN2) {
        GemmLn2Args g2{Ahi, lin.k16.hi, lin.w8, lin.bias, nrm.gamma, nrm.beta, ln.Xh, Xl8, M, K, 1e-5f, h->range_flag, no_lo_out};
        ProfScope ps(h, cls, ln.stream);
        HIPCHK(h, launch_gemm_ln2_mx(g2, rp.ln_rows, ln.stream));
        return 0;
    }
    if (rp.path == RB_GEMM_LN) {
        GemmLnArgs gl{Ahi, Alo, lin.k16.hi, lin.k16.lo, lin.bias, nrm.gamma, nrm.beta, ln.Xh, ln.Xl, M, K, 1e-5f, h->range_flag, p.mode.x2};
        gl.W8 = p.mode.mx ? lin.w8 : nullptr;
        gl.no_lo_out = p.mode.x2 && no_lo_out;
        ProfScope ps(h, cls, ln.stream);
        HIPCHK(h, launch_gemm_ln(gl, rp.ln_rows, ln.stream));
        return 0;
    }
    GemmHArgs g = gemm_h_args(p.mode, p.rm, M, Ahi, Alo, lin, d, K);
    g.C = ln.Y; g.ldc = d;
    if (rp.path == RB_LNX_SMALL) {
        if (rp.merge) {
            g.cmb_O = ln.Opart; g.cmb_ML = ln.MLpart; g.cmb_ns = p.cf.attn_nsplit; g.cmb_nhead = h->nhead;
            g.cmb_Mtot = (unsigned)((size_t)p.sg.nseq * p.sg.S);
        }
        g.ln_gamma = nrm.gamma; g.ln_beta = nrm.beta; g.ln_xh = ln.Xh; g.ln_xl = nullptr;
        g.ln_xl8 = Xl8; g.ln_xchg = ln.ln_xchg; g.ln_eps = 1e-5f; g.ln_no_lo = no_lo_out;
        return run_gemm_lnx_small(h, ln.stream, cls, g, rp.gemm);
    }
    if (int rc = (run_gemm_h<EPI_BIAS, OUT_F32>(h, ln.stream, cls, g, rp.gemm))) return rc;
    return run_add_ln(h, ln.stream, ln.X, ln.Y, nrm.gamma, nrm.beta, M, d, ln.Xh, ln.Xl, p.mxv2, no_lo_out);
}

// Steps one coefficient table of a chunk holds: all of the call's - built once per chunk - or one, rebuilt at the head of every step.
// From (steps, Ec, A, d) only.  The table is DEVICE MEMORY the handle's arena grows by, per chunk lane: 48 d bytes per (step, episode,
// agent) - the rows [.., 3, d] and their image [.., 3, 3 d] in fp32.  256 episodes of 5 agents at 50 steps and d_model 512 run as
// 43-episode chunks: 264 MB per lane, 528 MB with two chunks in flight, next to ~1.5 GB of step workspace.  kQkv0TableMaxBytes per lane
// caps it: a call beyond (a 100-step DDPM schedule on the same batch) keeps one step's table, 48 d Ec A bytes, and pays the small
// GEMM every step.
constexpr size_t kQkv0TableMaxBytes = size_t(512) << 20;
int qkv0_table_steps(int steps, int Ec, int A, int d) {
    const size_t bytes = (size_t)steps * Ec * A * 3 * 4 * d * sizeof(float);
    return bytes <= kQkv0TableMaxBytes ? steps : 1;
}

// The table of `nsteps` steps from step `step0` on for the chunk whose hyper rows are hyp_chunk: the coefficient rows, then in_proj
// of layer 0 on them in exact fp32 with per-tile sums (a row stands for every token of its (episode, agent) pair).
int qkv0_build_table(jmid_ctx* h, const StepPlan& p, const Lane& ln, const float* hyp_chunk, int step0, int nsteps) {
    const int d = h->d;
    ProfScope ps(h, KC_HYPER, ln.stream);
    Qkv0CoefArgs ca{h->wt.concat1.W, h->wt.concat1.bias, hyp_chunk, p.thyp(step0), ln.coef,
                    nsteps, p.R, d, h->hl.total, h->hl.g1, h->hl.b1, h->range_flag};
    const long total = (long)nsteps * p.R * (d / 4);
    hipLaunchKernelGGL(qkv0_coef_kernel, dim3((int)std::min<long>((total + 255) / 256, 256L * 16)), dim3(256), 0, ln.stream, ca);
    HIPCHK(h, hipGetLastError());
    GemmArgs g{};
    g.A = ln.coef; g.lda = d; g.W = h->wt.layers[0].in_proj.W; g.ldw = d; g.C = ln.uvc; g.ldc = 3 * d;
    g.M = nsteps * p.R * 3; g.N = 3 * d; g.K = d;
    if (h->tune.qkv0 == 2) HIPCHK(h, (launch_gemm_f32<EPI_BIAS, false>(g, ln.stream)));      // (A/B: what the per-tile sums buy)
    else HIPCHK(h, (launch_gemm_f32<EPI_BIAS, true>(g, ln.stream)));
    return 0;
}

// The folded tail's table is capped the same way, per chunk lane: (2 d + 2) floats per (step, episode, agent) - 44 MB for a 43-episode
// chunk of 5 agents at 50 steps and d_model 512.  Beyond the cap, and wherever a single step runs (jmid_net_eval), the table holds
// one step and is rebuilt at the head of each.  An entry is the same bits either way (tail_fold_table_kernel).
constexpr size_t kTailTableMaxBytes = size_t(128) << 20;
int tail_table_steps(int steps, int Ec, int A, int d) {
    const size_t bytes = (size_t)steps * Ec * A * (2 * d + 2) * sizeof(float);
    return bytes <= kTailTableMaxBytes ? steps : 1;
}

int tail_build_table(jmid_ctx* h, const StepPlan& p, const Lane& ln, const float* hyp_chunk, int step0, int nsteps) {
    const WeightTable& wt = h->wt;
    ProfScope ps(h, KC_HYPER, ln.stream);
    TailTableArgs ta{wt.concat3.W, wt.concat3.bias, wt.concat4.W, wt.concat4.bias, wt.linear.W, wt.linear.bias,
                     hyp_chunk, p.thyp(step0), ln.weff, ln.beff,
                     nsteps, p.R, h->d, h->dmid, h->dlow, h->hl.total,
                     h->hl.g3, h->hl.b3, h->hl.g4, h->hl.b4, h->hl.go, h->hl.bo, h->range_flag};
    HIPCHK(h, launch_tail_fold_table(ta, ln.stream));
    return 0;
}

EmbedArgs embed_args(const jmid_ctx* h, const StepPlan& p, const StepBuffers& sb, const float* x_chunk, const float* hyp_chunk, const float* th) {
    unsigned char* Xl8 = p.mxv2 ? reinterpret_cast<unsigned char*>(sb.Xl) : nullptr;
    return EmbedArgs{x_chunk, h->wt.concat1.W, h->wt.concat1.bias, h->pe, hyp_chunk, th,
                     p.mode.split ? nullptr : sb.X, p.M, h->d, h->hl.total, h->hl.g1, h->hl.b1, p.rm, p.mode.split ? sb.Xh : nullptr,
                     p.mode.split && !p.mxv2 ? sb.Xl : nullptr, Xl8};
}

int run_embed(jmid_ctx* h, const StepPlan& p, const Lane& ln, const float* x_chunk, const float* hyp_chunk, const float* thyp) {
    ProfScope ps(h, KC_EMBED, ln.stream);
    EmbedArgs ea = embed_args(h, p, ln, x_chunk, hyp_chunk, thyp);
    const long total = (long)p.M * (h->d / 4);
    int blocks = (int)std::min<long>((total + 255) / 256, 256L * 16);
    hipLaunchKernelGGL(embed_kernel, dim3(blocks), dim3(256), bystander_lds(h->tune.bystander_lds, embed_kernel), ln.stream, ea);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The bf8 images that replace the fp16 K_lo / Q_lo planes (plan_step: k8, q8l), in those planes' memory
struct LoImages {
    unsigned char *k8h, *k8l, *q8l;
};
LoImages lo_images(const StepPlan& p, const StepBuffers& sb, int d) {
    LoImages im{};
    im.k8h = p.k8 ? reinterpret_cast<unsigned char*>(sb.Kl) : nullptr;
    im.k8l = p.k8 ? im.k8h + (size_t)p.M * d : nullptr;
    im.q8l = p.q8l ? reinterpret_cast<unsigned char*>(sb.Ql) : nullptr;
    return im;
}

// The Q / K / V^T operand planes of layer l of a JMID step from the in_proj GEMM on the residual stream's planes (+ the transpose where
// its epilogue does not write V^T itself)
int in_proj_planes(jmid_ctx* h, const StepPlan& p, const Lane& ln, int l) {
    const int M = p.M, d = h->d, hd = p.hd, S = p.sg.S;
    const LoImages im = lo_images(p, ln, d);
    const float qscale = p.att_scale * 1.4426950408889634f;
    GemmHArgs g = gemm_h_args(p.mode, p.rm, M, ln.Xh, ln.Xl, h->wt.layers[l].in_proj, 3 * d, d);
    g.Chi = ln.Qh; g.Clo = ln.Ql; g.Khi = ln.Kh; g.Klo = ln.Kl;
    g.Vthi = p.vt_direct ? ln.Vth : ln.Vh; g.Vtlo = p.vt_direct ? ln.Vtl : ln.Vl; g.vt_direct = p.vt_direct;
    g.d = d; g.hd = hd; g.S = S; g.Spad = p.sg.Spad; g.qscale = qscale;
    g.K8h = im.k8h; g.K8l = im.k8l; g.Q8l = im.q8l;
    if (int rc = (run_gemm_h<EPI_BIAS, OUT_QKV>(h, ln.stream, KC_GEMM_QKV, g, p.in_proj))) return rc;
    if (!p.vt_direct) {
        ProfScope ps(h, KC_VTRANS, ln.stream);
        hipLaunchKernelGGL(v_transpose_kernel, dim3((S + 63) / 64, d / 64, p.sg.nseq), dim3(256), 0, ln.stream,
                           ln.Vh, ln.Vl, ln.Vth, ln.Vtl, S, p.sg.Spad, d, hd);
        HIPCHK(h, hipGetLastError());
    }
    return 0;
}

// The Q / K / V^T operand planes of layer l of a JMID step in the split-fp16 modes: the in_proj GEMM (in_proj_planes), or for layer 0
// the expansion of the coefficient table (qkv0.hpp).
int qkv_planes(jmid_ctx* h, const StepPlan& p, const Lane& ln, int l, int step_idx, const float* x_chunk, const float* hyp_chunk) {
    const int M = p.M, d = h->d, hd = p.hd, S = p.sg.S;
    const LoImages im = lo_images(p, ln, d);
    const float qscale = p.att_scale * 1.4426950408889634f;
    if (l == 0 && p.qkv0) {
        if (p.cf.qkv0_steps <= 1)
            if (int rc = qkv0_build_table(h, p, ln, hyp_chunk, step_idx, 1)) return rc;
        Qkv0Args qa{};
        qa.x = x_chunk;
        qa.uvc = ln.uvc + (p.cf.qkv0_steps <= 1 ? 0 : (size_t)step_idx * p.R * 9 * d);
        qa.ppe = h->ppe;
        qa.Qh = ln.Qh; qa.Ql = ln.Ql; qa.Kh = ln.Kh; qa.Kl = ln.Kl; qa.Vth = ln.Vth; qa.Vtl = ln.Vtl;
        qa.Q8l = im.q8l; qa.K8h = im.k8h; qa.K8l = im.k8l;
        qa.M = M; qa.d = d; qa.hd = hd; qa.S = S; qa.Spad = p.sg.Spad; qa.nseq = p.sg.nseq;
        qa.qscale = qscale; qa.rmap = p.rm; qa.range_flag = h->range_flag; qa.x2 = p.mode.x2;
        qkv0_plan(qa, p.T);
        ProfScope ps(h, KC_GEMM_QKV, ln.stream);
        HIPCHK(h, launch_qkv0_expand(qa, ln.stream));
        return 0;
    }
    return in_proj_planes(h, p, ln, l);
}

// The sampler's part of the output stage of step `step_idx`: what out_ddim*_kernel and tail_fold*_kernel share
OutArgs sampler_args(const jmid_ctx* h, const StepPlan& p, const StepBuffers& sb, int step_idx, float* x_chunk, const float* hyp_chunk,
                     float* e_out, const float* z_chunk) {
    OutArgs oa{sb.Y4, h->wt.linear.W, h->wt.linear.bias, hyp_chunk, p.thyp(step_idx), x_chunk, e_out,
               p.M, h->dlow, h->hl.total, h->hl.go, h->hl.bo,
               h->c_e[step_idx], h->c_x[step_idx], h->n_x[step_idx], h->n_e[step_idx], p.rm,
               nullptr, 0, 0.f, 0.f, 0.f, p.tbo(hyp_chunk)};
    if (h->ddpm && !e_out) {
        oa.ddpm = 1;
        oa.z = h->p_noise[step_idx] ? z_chunk : nullptr;
        oa.c0 = h->p_c0[step_idx];
        oa.c1 = h->p_c1[step_idx];
        oa.sigma = h->p_sigma[step_idx];
    }
    return oa;
}

// The tail of a step in the split-fp16 modes without its GEMMs (tail_fold.hpp): two dot products per token with the (row, step)'s
// 2 x d map, then the sampler update and the next step's embedding - one launch, one wave per trajectory piece or per token
// (StepPlan::out_tpw, as out_ddim*_kernel).  F16X3 reads X_hi + X_lo as its concat3 does, the other modes X_hi.
int folded_tail(jmid_ctx* h, const StepPlan& p, const Lane& ln, int step_idx, float* x_chunk, const float* hyp_chunk,
                float* e_out, const float* z_chunk, int next_step) {
    const int M = p.M, d = h->d;
    if (p.cf.tail_steps <= 1)
        if (int rc = tail_build_table(h, p, ln, hyp_chunk, step_idx, 1)) return rc;
    const size_t at = p.cf.tail_steps <= 1 ? 0 : (size_t)step_idx * p.R;
    const TailFoldArgs fa{ln.Xh, ln.Xl, ln.weff + at * 2 * d, ln.beff + at * 2, d};
    const OutArgs oa = sampler_args(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk);
    const bool embed_next = next_step >= 0 && !e_out;
    const EmbedArgs en = embed_next ? embed_args(h, p, ln, x_chunk, hyp_chunk, p.thyp(next_step)) : EmbedArgs{};
    const bool lo = !p.mode.x2;
    ProfScope ps(h, KC_OUT_DDIM, ln.stream);
    const auto launch = [&](auto* kernel, int waves, auto... tpw) {
        hipLaunchKernelGGL(kernel, dim3((waves + 3) / 4), dim3(256), bystander_lds(h->tune.bystander_lds, kernel), ln.stream, fa, oa, en, tpw...);
    };
    const auto pick = [&](auto embed, auto with_lo) {
        constexpr bool EN = decltype(embed)::value, LO = decltype(with_lo)::value;
        if (p.out_tpw) launch(tail_fold_traj_kernel<EN, LO>, M / p.out_tpw, p.out_tpw);
        else launch(tail_fold_kernel<EN, LO>, M);
    };
    if (embed_next && lo) pick(std::true_type{}, std::true_type{});
    else if (embed_next) pick(std::true_type{}, std::false_type{});
    else if (lo) pick(std::false_type{}, std::true_type{});
    else pick(std::false_type{}, std::false_type{});
    HIPCHK(h, hipGetLastError());
    return 0;
}

// output layer + sampler update (or e_theta out) + the next step's embedding on the Y4 rows the tail GEMMs left
int output_stage(jmid_ctx* h, const StepPlan& p, const Lane& ln, int step_idx, float* x_chunk, const float* hyp_chunk,
                 float* e_out, const float* z_chunk, int next_step) {
    const int M = p.M;
    ProfScope ps(h, KC_OUT_DDIM, ln.stream);
    const OutArgs oa = sampler_args(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk);
    const bool embed_next = next_step >= 0 && !e_out;
    const EmbedArgs en = embed_next ? embed_args(h, p, ln, x_chunk, hyp_chunk, p.thyp(next_step)) : EmbedArgs{};
    // four waves per workgroup: one wave per piece of a trajectory (out_tpw tokens), or one per token
    const auto launch = [&](auto* kernel, int waves, auto... tpw) {
        hipLaunchKernelGGL(kernel, dim3((waves + 3) / 4), dim3(256), bystander_lds(h->tune.bystander_lds, kernel), ln.stream, oa, en, tpw...);
    };
    if (p.out_tpw && embed_next) launch(out_ddim_traj_kernel<true>, M / p.out_tpw, p.out_tpw);
    else if (p.out_tpw) launch(out_ddim_traj_kernel<false>, M / p.out_tpw, p.out_tpw);
    else if (embed_next) launch(out_ddim_kernel<true>, M);
    else launch(out_ddim_kernel<false>, M);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The tail of a step in the split-fp16 modes on the residual stream's planes: folded (tail_fold.hpp), or
// concat3 -> concat4 as two launches, the output layer + sampler update + next embedding as a third (one fused kernel for all
// three was built in round 3 and measured slower at every batch size: docs/NOTEBOOK.md)
int net_tail(jmid_ctx* h, const StepPlan& p, const Lane& ln, int step_idx, float* x_chunk, const float* hyp_chunk,
             float* e_out, const float* z_chunk, int next_step) {
    if (p.tail_fold) return folded_tail(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk, next_step);
    const int M = p.M, d = h->d;
    const WeightTable& wt = h->wt;
    const float* thyp = p.thyp(step_idx);
    GemmHArgs g = gemm_h_args(p.mode, p.rm, M, ln.Xh, ln.Xl, wt.concat3, h->dmid, d);
    g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total;
    g.Chi = ln.Y3h; g.Clo = ln.Y3l; g.ldc = h->dmid; g.goff = h->hl.g3; g.boff = h->hl.b3;
    if (int rc = (run_gemm_h<EPI_CSL, OUT_SPLIT>(h, ln.stream, KC_GEMM_TAIL, g, p.concat3))) return rc;
    g = gemm_h_args(p.mode, p.rm, M, ln.Y3h, ln.Y3l, wt.concat4, h->dlow, h->dmid);
    g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total;
    g.C = ln.Y4; g.ldc = h->dlow; g.goff = h->hl.g4; g.boff = h->hl.b4;
    if (int rc = (run_gemm_h<EPI_CSL, OUT_F32>(h, ln.stream, KC_GEMM_TAIL, g, p.concat4))) return rc;
    return output_stage(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk, next_step);
}

// one evaluation of the net on a chunk of whole episodes + (optionally) the DDIM update, as its plan says
// (dbg_layer below repeats the body of the layer loop launch for launch, with a read-back after every stage: a change here belongs there too)
int net_step(jmid_ctx* h, const StepPlan& p, const Lane& ln, int step_idx, float* x_chunk, const float* hyp_chunk,
             float* e_out, const float* z_chunk = nullptr, bool embed_done = false, int next_step = -1, const unsigned* mask_chunk = nullptr) {
    // mask_chunk: the key-mask words of the chunk's episodes in a padded call (p.attn.masked), else null
    // embed_done: the previous step's output kernel already embedded x for this step; next_step >= 0: this step's
    // output kernel does the same for step `next_step` (same chunk, same buffers)
    const bool split = p.mode.split;
    const int M = p.M, d = h->d, ff = h->ff;
    const WeightTable& wt = h->wt;
    const float* thyp = p.thyp(step_idx);
    const RowMap& rm = p.rm;
    if (!embed_done)
        if (int rc = run_embed(h, p, ln, x_chunk, hyp_chunk, thyp)) return rc;
    const SeqGeom& sg = p.sg;
    const int nseq = sg.nseq, S = sg.S, hd = p.hd;
    if (!split) {
        for (const LayerW& w : wt.layers) {
            if (int rc = run_gemm<EPI_BIAS>(h, ln.stream, KC_GEMM_QKV, gemm_args(rm, M, ln.X, w.in_proj, ln.QKV, 3 * d, d))) return rc;
            {
                ProfScope ps(h, KC_ATTN, ln.stream);
                AttnArgs aa{ln.QKV, ln.ATT, S, d, h->nhead, p.att_scale, nullptr, nullptr};
                aa.mask = p.attn.masked ? mask_chunk : nullptr;
                HIPCHK(h, launch_attn_f32(aa, nseq, hd, p.attn.pack, ln.stream));
            }
            // attention output projection + residual + LN1
            if (int rc = run_gemm<EPI_BIAS>(h, ln.stream, KC_GEMM_OUT, gemm_args(rm, M, ln.ATT, w.out_proj, ln.Y, d, d))) return rc;
            if (int rc = run_add_ln(h, ln.stream, ln.X, ln.Y, w.norm1.gamma, w.norm1.beta, M, d)) return rc;
            // feed-forward
            if (int rc = run_gemm<EPI_BIAS_RELU>(h, ln.stream, KC_GEMM_FF1, gemm_args(rm, M, ln.X, w.linear1, ln.H1, ff, d))) return rc;
            if (int rc = run_gemm<EPI_BIAS>(h, ln.stream, KC_GEMM_FF2, gemm_args(rm, M, ln.H1, w.linear2, ln.Y, d, ff))) return rc;
            if (int rc = run_add_ln(h, ln.stream, ln.X, ln.Y, w.norm2.gamma, w.norm2.beta, M, d)) return rc;
        }
        // tail: concat3, concat4 (ConcatSquash epilogues)
        GemmArgs g = gemm_args(rm, M, ln.X, wt.concat3, ln.Y3, h->dmid, d);
        g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total; g.goff = h->hl.g3; g.boff = h->hl.b3;
        if (int rc = run_gemm<EPI_CSL>(h, ln.stream, KC_GEMM_TAIL, g)) return rc;
        g = gemm_args(rm, M, ln.Y3, wt.concat4, ln.Y4, h->dlow, h->dmid);
        g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total; g.goff = h->hl.g4; g.boff = h->hl.b4;
        if (int rc = run_gemm<EPI_CSL>(h, ln.stream, KC_GEMM_TAIL, g)) return rc;
    } else {
        for (int l = 0; l < h->tf_layer; ++l) {
            const LayerW& w = wt.layers[l];
            GemmHArgs g{};
            if (p.joint) {
                if (int rc = qkv_planes(h, p, ln, l, step_idx, x_chunk, hyp_chunk)) return rc;
                const LoImages im = lo_images(p, ln, d);
                ProfScope ps(h, KC_ATTN, ln.stream);
                AttnHArgs aa{ln.Qh, ln.Ql, ln.Kh, ln.Kl, ln.Vth, ln.Vtl, ln.Ah, ln.Al, S, sg.Spad, d, h->nhead,
                             p.att_scale, h->range_flag, p.cf.attn_nsplit, ln.Opart, ln.MLpart, p.mode.x2, im.k8h, im.k8l, im.q8l};
                aa.skip_combine = p.out_proj.merge;
                HIPCHK(h, launch_attn_f16x3(aa, nseq, hd, p.attn, ln.stream, p.attn.masked ? mask_chunk : nullptr));
            } else {
                g = gemm_h_args(p.mode, rm, M, ln.Xh, ln.Xl, w.in_proj, 3 * d, d);
                g.C = ln.QKV; g.ldc = 3 * d;
                if (int rc = (run_gemm_h<EPI_BIAS, OUT_F32>(h, ln.stream, KC_GEMM_QKV, g, p.in_proj))) return rc;
                ProfScope ps(h, KC_ATTN, ln.stream);
                AttnArgs aa{ln.QKV, nullptr, S, d, h->nhead, p.att_scale, ln.Ah, ln.Al};
                HIPCHK(h, launch_attn_f32(aa, nseq, hd, p.attn.pack, ln.stream));
            }
            if (int rc = residual_block(h, p, p.out_proj, ln, ln.Ah, ln.Al, d, w.out_proj, w.norm1, KC_GEMM_OUT, false)) return rc;
            g = gemm_h_args(p.mode, rm, M, ln.Xh, ln.Xl, w.linear1, ff, d);
            g.Chi = ln.H1h; g.Clo = ln.H1l; g.ldc = ff;
            if (int rc = (run_gemm_h<EPI_BIAS_RELU, OUT_SPLIT>(h, ln.stream, KC_GEMM_FF1, g, p.linear1))) return rc;
            // (the residual stream ends with the last layer: concat3 reads X_hi only)
            if (int rc = residual_block(h, p, p.linear2, ln, ln.H1h, ln.H1l, ff, w.linear2, w.norm2, KC_GEMM_FF2, l + 1 == h->tf_layer)) return rc;
        }
        return net_tail(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk, next_step);
    }
    return output_stage(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk, next_step);
}

// Episodes per pass of the 50-step loop when nothing is forced: large enough to fill the chip several times over per
// launch, and - for JMID - a whole number of "rounds" of the attention launch: that kernel runs 2 workgroups per CU
// (512 slots) and one episode contributes nhead * ceil(S/128) workgroups, so a chunk of floor(k*512 / that) episodes
// leaves no partially filled last round (20 -> 51 episodes: +15 % attention throughput on BASELINE cfg3).
int auto_chunk(const jmid_ctx* h, int E, int tokens_per_episode) {
    const long max_tokens = 65536;
    if (h->net_kind == JMID_NET_JMID) {
        const long bpe = (long)h->nhead * ((tokens_per_episode + 127) / 128);
        for (int k = 4; k >= 1; --k) {
            const long c = (k * 512L) / bpe;
            if (c >= 1 && c * tokens_per_episode <= max_tokens) return (int)std::min<long>(c, E);
        }
    }
    long c = max_tokens / std::max(1, tokens_per_episode);
    if (c < 1) c = 1;
    return (int)std::min<long>(c, E);
}

// The chunks of a call: `c` episodes each (jmid_set_chunk_episodes, or auto_chunk).  A short ragged tail (less than a
// quarter of a chunk, e.g. 256 = 5 x 51 + 1) would run all 50 steps at single-scene latency, so it is spread over the
// full chunks instead (52 + 4 x 51) - only with the automatic size: a forced size is taken literally.
std::vector<int> plan_chunks(const jmid_ctx* h, const CallMode& m, int E, int tokens_per_episode) {
    int c = h->chunk_eps > 0 ? std::min(E, h->chunk_eps) : auto_chunk(h, E, tokens_per_episode);
    if (h->chunk_eps <= 0 && h->lanes >= 2 && E >= 2 && h->tune.graph != 1) {     // (a captured loop is a one-chunk call)
        // Two chunks in flight want an EVEN number of chunks of equal size.  A batch that fits one chunk is split in two halves: its
        // kernels do not fill the chip, and two half-size launches side by side finish 5-13 % sooner than one (4 / 8 / 16 / 32 / 48
        // episodes: 23.3 -> 22.2, 36.0 -> 31.8, 60.9 -> 58.0, 111.3 -> 97.2, 140.5 -> 132.5 ms per call; tools/small_batch_lanes.py).
        // A larger batch runs as the smallest even number of chunks that fit, balanced: 256 episodes = 4 x 43 + 2 x 42 instead of
        // 52 + 4 x 51 (an odd count leaves the last chunk alone on the chip) or, in JMID_PREC_F16MX until round 4, 10 x 26 -
        // with the leaner kernels of that round's last session the half-size chunks lost their edge: 256 episodes 564 -> 540 ms,
        // 512: 1142 -> 1086, 160: 356 -> 347, 104: 230 -> 224 (F16MX); F16X2 / F16X3 within 0.4 % either way (tools/chunk_fine.py).
        // The split-KV factor of a call does not depend on its chunk plan (run_network), so neither do the results.
        if (E <= c) {
            // ... unless the whole batch is at most 2 560 tokens in F16MX at d_model 512: as ONE chunk its out-projection / linear2 launches
            // carry the LayerNorm and the split-KV merge (gemm_small.hpp, OUT_LNX - only while nothing else of the handle is in flight),
            // nine launches less per denoise step: two cfg2 scenes (2 400 tokens) 14.45 -> 13.90 ms per call, 12.63 with the split-KV factor chosen for that launch (run_network).  Three (3 600 tokens, 456
            // workgroups of that kernel) are better off as 2 + 1 side by side: 16.42 against 16.90 (profiles/r05s_lnx_two_per_cu.log)
            const long tokens = (long)E * tokens_per_episode;
            const bool lnx_call = one_launch_shape(h, m, tokens) && residual_path(h, m, (int)tokens, h->d, CallFacts{}).path == RB_LNX_SMALL;
            c = lnx_call ? E : (E + 1) / 2;
        } else {
            int n = (E + c - 1) / c;
            if ((n & 1) && n < E) ++n;      // (never more chunks than episodes: c == 1 with an odd E stays at E chunks of one)
            std::vector<int> sizes(n, E / n);
            for (int i = 0; i < E % n; ++i) sizes[i] += 1;
            return sizes;
        }
    }
    std::vector<int> sizes(E / c, c);
    const int tail = E % c;
    if (tail) {
        if (h->chunk_eps > 0 || sizes.empty() || tail * 4 >= c || (tail + sizes.size() - 1) / sizes.size() > (size_t)c / 8)
            sizes.push_back(tail);
        else
            for (int i = 0; i < tail; ++i) sizes[i % sizes.size()] += 1;
    }
    return sizes;
}

// Device-mode calls read and write the caller's buffers on the handle's private stream.  They are ordered against
// the stream the caller works on (jmid_set_caller_stream; default: the legacy null stream): the handle's stream waits
// for everything the caller enqueued before the call, and the caller's stream waits for the call's last kernel, so
// neither a producer kernel of an input nor a consumer (or the allocator's reuse) of an output can race with it.
int order_in(jmid_ctx* h, int mem) {
    if (mem != JMID_MEM_DEVICE) return 0;
    HIPCHK(h, hipEventRecord(h->ev_in, h->caller_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_in, 0));
    return 0;
}
int order_out(jmid_ctx* h, int mem) {
    if (mem != JMID_MEM_DEVICE) return 0;
    HIPCHK(h, hipEventRecord(h->ev_out, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->caller_stream, h->ev_out, 0));
    return 0;
}

int check_ready(jmid_ctx* h) {
    if (!h) return JMID_EINVAL;
    if (!h->finalized) return fail(h, JMID_ENOWEIGHT, "jmid_finalize_weights has not been called");
    if (h->beta.empty() || !h->thyp) return fail(h, JMID_EINVAL, "jmid_set_ddim_table has not been called");
    return 0;
}

int check_n_agents(jmid_ctx* h, const char* who, const int32_t* n_agents, int E, int A) {
    if (!n_agents) return fail(h, JMID_EINVAL, std::string(who) + ": null n_agents");
    for (int e = 0; e < E; ++e)
        if (n_agents[e] < 1 || n_agents[e] > A)
            return fail(h, JMID_EINVAL, std::string(who) + ": n_agents[" + std::to_string(e) + "] = " + std::to_string(n_agents[e]) + " is outside 1..A");
    return 0;
}

// One draw for E episodes of n elements each (noise.hpp): normals to `out` and / or the raw words to `words`, device buffers.
int fill_noise(jmid_ctx* h, uint64_t seed, const unsigned* ids_dev, int E, size_t n, int draw, float* out, unsigned* words, hipStream_t stream) {
    NoiseArgs g{};
    g.ids = ids_dev; g.out = out; g.words = words;
    g.n = n; g.E = E;
    g.key0 = (unsigned)(seed & 0xffffffffull); g.key1 = (unsigned)(seed >> 32);
    g.draw = (unsigned)draw;
    HIPCHK(h, launch_noise(g, stream));
    return 0;
}

int fill_noise_padded(jmid_ctx* h, uint64_t seed, const unsigned* ids_dev, const int* n_agents_dev, int E, int A, int K, int T, int draw, float* out,
                      hipStream_t stream) {
    NoisePaddedArgs g{};
    g.ids = ids_dev; g.n_agents = n_agents_dev; g.out = out;
    g.key0 = (unsigned)(seed & 0xffffffffull); g.key1 = (unsigned)(seed >> 32);
    g.draw = (unsigned)draw;
    g.E = E; g.A = A; g.K = K; g.T = T;
    HIPCHK(h, launch_noise_padded(g, stream));
    return 0;
}

// Everything a denoise call decides, decided before it enqueues anything: host values only.  The phases of run_network read it;
// net_step executes its step plans.
struct CallPlan {
    CallMode mode;
    std::vector<int> chunk_sizes, chunk_start;      // episodes of each chunk (plan_chunks) and its first episode
    size_t Mc;                                      // tokens of the largest chunk: what a lane's step workspace holds
    SeqGeom sg;                                     // ... and its attention geometry
    // Independent chunks run `nlanes` at a time on separate streams: the partially filled last round of one chunk's
    // kernels and its bandwidth-bound kernels overlap with another chunk's MFMA kernels.  Each lane has its own step
    // workspace; results do not depend on the number of lanes.
    int nlanes;
    Lane lanes[jmid_ctx::kMaxLanes];                // (their buffers: fill_workspace)
    CallFacts facts;
    // one plan per distinct chunk size of the call (the knobs and lnx_off cannot change while it runs): a handful at most
    std::vector<StepPlan> plans;
    std::vector<int> chunk_plan;                    // chunk -> its plan
    size_t qkv0_rows, tail_rows;                    // rows of a lane's two tables (step_ws_floats)
    bool masked;                                    // a padded call (DenoiseCall::n_agents)
    bool z_fill;                                    // seeded DDPM: the z of ONE step per lane, filled on that lane's stream just before the step's update (no [n_steps, ...] buffer)
};

CallPlan plan_call(const jmid_ctx* h, const DenoiseCall& a, const CallMode& mode) {
    const int E = a.E, A = a.A, K = a.K, T = a.T;
    CallPlan cp{};
    cp.mode = mode;
    cp.masked = a.n_agents != nullptr;
    cp.chunk_sizes = plan_chunks(h, mode, E, K * A * T);
    cp.chunk_start.assign(cp.chunk_sizes.size(), 0);
    for (size_t i = 1; i < cp.chunk_sizes.size(); ++i) cp.chunk_start[i] = cp.chunk_start[i - 1] + cp.chunk_sizes[i - 1];
    const int Ec = *std::max_element(cp.chunk_sizes.begin(), cp.chunk_sizes.end());
    cp.Mc = (size_t)Ec * K * A * T;
    cp.sg = seq_geom(h, Ec, A, K, T);
    // Split-KV factor of the attention launches: chosen ONCE per call from the automatic chunk size, never from the
    // chunk at hand - a ragged last chunk or a forced chunk size must not change the order in which a sequence's keys
    // are summed (results are bit-identical for every chunking of the same call).
    int ns_call = 1;
    if (h->net_kind == JMID_NET_JMID && mode.split && h->d / h->nhead == 128) {
        const int S = K * A * T;
        // sized for ONE launch of the default plan (two chunks in flight: a batch that fits one chunk runs as two halves) - a
        // function of the call's shape only, whatever the chunk size or number of lanes actually set
        const int c_auto = auto_chunk(h, E, S);
        // (a batch of at most 2 560 tokens in F16MX is ONE launch by default - plan_chunks: two cfg2 scenes take 3 key ranges x 80 blocks,
        //  13.43 ms per call, where the 6 x 80 of the halves' choice take 14.14-14.37; shape and mode only, no knob: the bits of a call
        //  must not depend on one)
        ns_call = attn_pick_nsplit(((S + 127) / 128) * h->nhead * (E >= 2 ? (one_launch_shape(h, mode, (long)E * S) ? E : (c_auto + 1) / 2) : 1), S);
        if (h->tune.attn_nsplit > 0) ns_call = std::min(h->tune.attn_nsplit, (S + 31) / 32);
    }
    cp.nlanes = a.single_step < 0 ? std::max(1, std::min(h->lanes, (int)cp.chunk_sizes.size())) : 1;
    for (int l = 0; l < cp.nlanes; ++l) cp.lanes[l].stream = l ? h->lane_stream[l - 1] : h->stream;
    cp.z_fill = a.seeded && h->ddpm && a.single_step < 0;
    // The small-launch GEMMs (gemm_small.hpp: one workgroup per CU, most of its LDS) only while one chunk is in flight
    cp.facts.small_now = cp.nlanes == 1 || h->tune.small_lanes == 1 ? 1 : h->tune.small_lanes == 2 ? 2 : 0;
    cp.facts.one_chunk = cp.chunk_sizes.size() == 1 && h->tune.graph != 1;      // (a captured loop would replay the launch tags of OUT_LNX)
    cp.facts.attn_nsplit = ns_call;
    const int n_steps = (int)h->beta.size();
    cp.facts.qkv0_steps = a.single_step < 0 ? qkv0_table_steps(n_steps, Ec, A, h->d) : 1;
    cp.facts.tail_steps = a.single_step < 0 && h->tune.tail_fold != 2 ? tail_table_steps(n_steps, Ec, A, h->d) : 1;
    for (int ec : cp.chunk_sizes) {
        size_t j = 0;
        while (j < cp.plans.size() && cp.plans[j].Ec != ec) ++j;
        if (j == cp.plans.size()) cp.plans.push_back(plan_step(h, ec, A, K, T, mode, cp.facts, cp.masked));
        cp.chunk_plan.push_back((int)j);
    }
    if (a.loss)      // the rows' timesteps are inside hyp (loss_prepare_kernel): a zero row for the one "step"
        for (StepPlan& p : cp.plans) p.thyp_base = h->zero_thyp, p.thyp_stride = 0;
    cp.qkv0_rows = cp.plans[0].qkv0 ? (size_t)cp.facts.qkv0_steps * Ec * A * 3 : 0;
    cp.tail_rows = cp.plans[0].tail_fold ? (size_t)cp.facts.tail_steps * Ec * A : 0;
    return cp;
}

// The I/O block of a call's workspace, in front of the lanes' step workspaces.  base null: its size only (as step_ws_floats).
struct CallIo {
    float *x_cur, *ctx, *hyp, *p0, *stage, *z_up, *z_lane;      // stage: e / pos; z_up: the caller's DDPM noise; z_lane: z_fill
    unsigned* mask;      // a padded JMID call: key-mask words [E][ceil(S / 32)] (padded.hpp) - a chunk's words are its episodes' slice
    const int* nag;      // ... and every padded call: its counts on the device (h->nag's upload, or DenoiseCall::n_agents_dev)
    // a loss call (loss.hpp): e where it is not the caller's device array (its upload, or the seeded draw), the per-row sums, {loss, count}
    float* e_up;
    float* tbo;          // (StepPlan::loss_tbo; only off the folded tail)
    double *loss_rows, *loss;
    const float* e_dev;  // ... and the e the two loss kernels read (fill_workspace)
    float* guide;        // a guided call: [E, K, 2] the rows the guide kernel accumulates over the steps, zeroed by fill_workspace
};
size_t call_io(const jmid_ctx* h, const DenoiseCall& a, const CallPlan& cp, char* base, CallIo* out) {
    const size_t M = (size_t)a.E * a.K * a.A * a.T, EA = (size_t)a.E * a.A;
    Carver c(base);
    CallIo io{};
    io.x_cur = c.take(M * 2);
    io.ctx = c.take(EA * h->ctx_dim);
    io.hyp = c.take(EA * h->hl.total);
    io.p0 = c.take(EA * 2);
    io.stage = c.take(M * 2);
    if (a.z && a.mem == JMID_MEM_HOST) io.z_up = c.take(M * 2 * h->beta.size());
    if (cp.z_fill) io.z_lane = c.take((size_t)cp.nlanes * cp.Mc * 2);
    if (cp.masked && h->net_kind == JMID_NET_JMID) io.mask = reinterpret_cast<unsigned*>(c.take((size_t)a.E * mask_words_per_seq(a.K * a.A * a.T)));
    if (a.loss) {
        if (!a.loss->e || a.mem == JMID_MEM_HOST) io.e_up = c.take(M * 2);
        if (!cp.plans[0].tail_fold) io.tbo = c.take(EA * 2);
        io.loss_rows = c.take<double>(EA);
        io.loss = c.take<double>(2);
    }
    if (a.guide) io.guide = c.take((size_t)a.E * a.K * GDE_COLS);
    if (out) *out = io;
    return c.off;
}

int check_call(jmid_ctx* h, const DenoiseCall& a, CallMode* mode) {
    if (int rc = check_ready(h)) return rc;
    if (a.E <= 0 || a.A <= 0 || a.K <= 0 || a.T <= 0) return fail(h, JMID_EINVAL, "E, A, K, T must be positive");
    if (a.T > kPeMaxLen) return fail(h, JMID_EINVAL, "T exceeds the positional-encoding table (max_len=24, diffusion.py:116-118)");
    if (!call_mode(a.precision, mode))
        return fail(h, JMID_EINVAL, "precision must be JMID_PREC_F32, JMID_PREC_F16X3, JMID_PREC_F16X2 or JMID_PREC_F16MX (JMID_PREC_F16 is not built)");
    if (mode->split && !h->weights_in_half_range && ++h->erange_calls)
        return fail(h, JMID_ERANGE, "a weight exceeds the fp16 range: use JMID_PREC_F32");
    if ((!a.x_in && !a.seeded) || !a.ctx) return fail(h, JMID_EINVAL, "null input");
    if (a.seeded && !a.seeded->ids) return fail(h, JMID_EINVAL, "null episode_ids");
    if (a.seeded && !noise_fits((unsigned long long)a.K * a.A * a.T * 2)) return fail(h, JMID_EINVAL, "K * A * T exceeds the noise addressing");
    if (a.pos_out && !a.p0) return fail(h, JMID_EINVAL, "pos_out requested without p0");
    if (a.n_agents) {
        if (a.z || (a.single_step < 0 && h->ddpm)) return fail(h, JMID_EINVAL, "a padded call samples with DDIM only");
        if (int rc = check_n_agents(h, "padded call", a.n_agents, a.E, a.A)) return rc;
        if (h->net_kind == JMID_NET_JMID && mode->split && !attn_masked_built(plan_attn(h->d / h->nhead, h->tune), mode->x2 != 0))
            return fail(h, JMID_EINVAL, "a padded call needs the default attention kernel: \"attn_sm\" = 2 and the ablations (every split mode), \"attn_mx\" = 1 and \"attn_pf\" = 2 (F16X2 / F16MX) have no masked form");
    }
    if (const LossCall* lc = a.loss) {
        const std::string w(a.who);
        if (a.K != 1 || a.single_step < 0) return fail(h, JMID_EINVAL, w + ": a loss call is one net evaluation with K = 1");
        if (!h->loss_tt) return fail(h, JMID_EINVAL, w + ": jmid_set_loss_schedule has not been called");
        if (!lc->t || !lc->loss_out || (!lc->e && !lc->seeded)) return fail(h, JMID_EINVAL, w + ": null argument");
        if (lc->seeded && !lc->seeded->ids) return fail(h, JMID_EINVAL, w + ": null episode_ids");
        if (lc->seeded && !noise_fits((unsigned long long)a.A * a.T * 2)) return fail(h, JMID_EINVAL, w + ": A * T exceeds the noise addressing");
        const int n_t = (int)h->loss_beta.size();
        for (size_t r = 0; r < (size_t)a.E * a.A; ++r)
            if (lc->t[r] < 1 || lc->t[r] >= n_t)
                return fail(h, JMID_EINVAL, w + ": t[" + std::to_string(r / a.A) + ", " + std::to_string(r % a.A) + "] = " + std::to_string(lc->t[r]) +
                                                " (row " + std::to_string(r) + ") is outside 1.." + std::to_string(n_t - 1));
    }
    if (const GuideCall* gc = a.guide) {
        const std::string w(a.who);
        if (a.single_step >= 0 || a.loss || a.z) return fail(h, JMID_EINVAL, w + ": a guided call is a DDIM denoise call");
        if (h->ddpm) return fail(h, JMID_EINVAL, w + ": a guided call samples with DDIM only (a DDPM table is installed)");
        if (!a.p0) return fail(h, JMID_EINVAL, w + ": null p0 (the guidance is defined on positions)");
        if (!(a.dt > 0.0f) || !std::isfinite(a.dt)) return fail(h, JMID_EINVAL, w + ": dt must be finite and > 0");
        if (!gc->weights) return fail(h, JMID_EINVAL, w + ": null weights");
        for (size_t i = 0; i < h->beta.size(); ++i)
            if (!(gc->weights[i] >= 0.0) || !std::isfinite(gc->weights[i]))
                return fail(h, JMID_EINVAL, w + ": weights[" + std::to_string(i) + "] must be finite and >= 0");
    }
    h->last_pos = nullptr;     // (the staging buffer is about to be reused)
    if (a.single_step < 0 && h->ddpm && !a.z && !a.seeded) return fail(h, JMID_EINVAL, "DDPM table installed: use jmid_denoise_ddpm (needs z)");
    if (a.single_step < 0 && !h->ddpm && a.z) return fail(h, JMID_EINVAL, "jmid_denoise_ddpm needs jmid_set_ddpm_table");
    return 0;
}

// Lay the workspace out (I/O block, then one step workspace per lane) and fill it on h->stream: uploads, memsets, the hyper nets'
// ctx part; the extra lanes fork behind all of it.  From here on a.z, a.ctx and a.p0 are device pointers: the caller's, or their uploads.
int fill_workspace(jmid_ctx* h, DenoiseCall& a, CallPlan& cp, CallIo& io) {
    const size_t M = (size_t)a.E * a.K * a.A * a.T, EA = (size_t)a.E * a.A;
    const size_t io_off = call_io(h, a, cp, nullptr, nullptr);
    const size_t lane_floats = step_ws_floats(h, cp.Mc, cp.mode, cp.sg, cp.facts.attn_nsplit, nullptr, nullptr, cp.qkv0_rows, cp.tail_rows);
    if (int rc = ensure_arena(h, io_off + cp.nlanes * lane_floats, a.who)) return rc;
    call_io(h, a, cp, h->arena.p, &io);
    for (int l = 0; l < cp.nlanes; ++l) {
        step_ws_floats(h, cp.Mc, cp.mode, cp.sg, cp.facts.attn_nsplit, &cp.lanes[l], h->arena.p + io_off + l * lane_floats, cp.qkv0_rows, cp.tail_rows);
        cp.lanes[l].z = cp.z_fill ? io.z_lane + (size_t)l * cp.Mc * 2 : nullptr;
    }
    if (io.z_up) {
        HIPCHK(h, hipMemcpyAsync(io.z_up, a.z, M * 2 * h->beta.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        a.z = io.z_up;
    }
    if (cp.mode.split) {
        HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), h->stream));
        for (int l = 0; l < cp.nlanes; ++l) HIPCHK(h, hipMemsetAsync(cp.lanes[l].ln_xchg, 0, kLnxWords * sizeof(unsigned), h->stream));
        for (int l = 0; l < cp.nlanes; ++l) {
            const StepBuffers& sb = cp.lanes[l];
            if (sb.Vth && cp.sg.Spad != cp.sg.S) {  // padding keys of V^T must be finite (they meet P = 0)
                HIPCHK(h, hipMemsetAsync(sb.Vth, 0, sb.vt_elems * sizeof(half_t), h->stream));
                HIPCHK(h, hipMemsetAsync(sb.Vtl, 0, sb.vt_elems * sizeof(half_t), h->stream));
            }
        }
    }
    const hipMemcpyKind kin = a.mem == JMID_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (cp.masked) {      // the counts first: a seeded padded fill addresses with them
        io.nag = a.n_agents_dev;
        if (!io.nag) {
            if (int rc = h->nag.upload(h, a.n_agents, a.E, a.who)) return rc;
            io.nag = h->nag.get<int>();
        }
    }
    if (a.seeded && cp.masked) {
        if (int rc = h->noise_ids.upload(h, a.seeded->ids, a.E, a.who)) return rc;
        if (int rc = fill_noise_padded(h, a.seeded->seed, h->noise_ids.get<unsigned>(), io.nag, a.E, a.A, a.K, a.T, a.seeded->draw, io.x_cur, h->stream)) return rc;
    } else if (a.seeded) {
        if (int rc = h->noise_ids.upload(h, a.seeded->ids, a.E, a.who)) return rc;
        if (int rc = fill_noise(h, a.seeded->seed, h->noise_ids.get<unsigned>(), a.E, (size_t)a.K * a.A * a.T * 2, a.seeded->draw, io.x_cur, nullptr, h->stream)) return rc;
    } else {
        HIPCHK(h, hipMemcpyAsync(io.x_cur, a.x_in, M * 2 * sizeof(float), kin, h->stream));
    }
    if (a.mem == JMID_MEM_HOST || cp.masked) {      // (a padded call zeroes rows of ctx and p0: never in the caller's arrays)
        HIPCHK(h, hipMemcpyAsync(io.ctx, a.ctx, EA * h->ctx_dim * sizeof(float), kin, h->stream));
        a.ctx = io.ctx;
    }
    if (a.p0 && (a.mem == JMID_MEM_HOST || cp.masked)) {
        HIPCHK(h, hipMemcpyAsync(io.p0, a.p0, EA * 2 * sizeof(float), kin, h->stream));
        a.p0 = io.p0;
    }
    if (cp.masked) {
        // the counts, the key-mask words from them, and zeros in the padded agents' rows of x_T, ctx and p0: whatever the caller left
        // there is never read.  All of it outside a captured loop, on memory the loop reads: a replay sees this call's counts.
        if (io.mask) HIPCHK(h, launch_mask_words(io.nag, io.mask, a.E, a.A, a.T, a.K * a.A * a.T, h->stream));
        HIPCHK(h, launch_pad_fill(io.x_cur, io.nag, a.E, a.K, a.A, a.T * 2, 0.f, h->stream));
        HIPCHK(h, launch_pad_fill(io.ctx, io.nag, a.E, 1, a.A, h->ctx_dim, 0.f, h->stream));
        if (a.p0) HIPCHK(h, launch_pad_fill(io.p0, io.nag, a.E, 1, a.A, 2, 0.f, h->stream));
    }
    // ---- ctx part of the four hyper nets, once per call (ctx is constant over the denoise steps)
    GemmArgs g{};
    g.A = a.ctx; g.lda = h->ctx_dim; g.W = h->Whyp; g.ldw = h->ctx_dim; g.bias = h->bhyp; g.C = io.hyp;
    g.ldc = h->hl.total; g.M = (int)EA; g.N = h->hl.total; g.K = h->ctx_dim;
    if (int rc = run_gemm<EPI_BIAS>(h, h->stream, KC_HYPER, g)) return rc;
    if (const LossCall* lc = a.loss) {
        // x_cur holds x0 (zeros in the padded rows): e to the device, then x_t in place and every row's timestep into its hyp row
        if (int rc = h->loss_t.upload(h, lc->t, (int)EA, a.who)) return rc;
        io.e_dev = io.e_up ? io.e_up : lc->e;
        if (!lc->e) {
            if (int rc = h->noise_ids.upload(h, lc->seeded->ids, a.E, a.who)) return rc;
            if (int rc = fill_noise(h, lc->seeded->seed, h->noise_ids.get<unsigned>(), a.E, (size_t)a.A * a.T * 2, 0, io.e_up, nullptr, h->stream)) return rc;
        } else if (io.e_up) {
            HIPCHK(h, hipMemcpyAsync(io.e_up, lc->e, M * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        const int n_t = (int)h->loss_beta.size();
        const LossPrepareArgs pa{io.x_cur, io.e_dev, h->loss_t.get<int>(), h->loss_c, h->loss_c + n_t, io.hyp, h->loss_tt,
                                 io.nag, io.tbo, (int)EA, a.A, a.T * 2, h->hl.total, h->hl.bo};
        for (StepPlan& p : cp.plans) p.loss_hyp = io.hyp, p.loss_tbo = io.tbo;
        ProfScope ps(h, KC_LOSS_PREPARE, h->stream);
        HIPCHK(h, launch_loss_prepare(pa, h->stream));
    }
    if (a.guide) HIPCHK(h, hipMemsetAsync(io.guide, 0, (size_t)a.E * a.K * GDE_COLS * sizeof(float), h->stream));
    if (cp.nlanes > 1) {   // everything enqueued so far (inputs, hyper nets, memsets) precedes the extra lanes as well
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        for (int l = 1; l < cp.nlanes; ++l) HIPCHK(h, hipStreamWaitEvent(cp.lanes[l].stream, h->ev_fork, 0));
    }
    return 0;
}

// The guide kernel (guide.hpp) on the episodes [el, el + ec) of a guided call, behind step-table entry i on the chunk's own stream
int guide_chunk(jmid_ctx* h, const DenoiseCall& a, const CallIo& io, const Lane& ln, int i, size_t el, int ec) {
    const GuideCall& gc = *a.guide;
    GuideArgs g{};
    g.x = io.x_cur + el * (size_t)a.K * a.A * a.T * 2;
    g.p0 = a.p0 + el * (size_t)a.A * 2;
    g.n_agents = io.nag ? io.nag + el : nullptr;
    g.walls = gc.walls;
    g.out = io.guide + el * (size_t)a.K * GDE_COLS;
    g.threshold = gc.threshold; g.margin = gc.margin; g.tau = gc.tau; g.weight = gc.weights[i]; g.dt = (double)a.dt;
    g.wall_radius = gc.wall_radius;
    g.E = ec; g.A = a.A; g.K = a.K; g.T = a.T; g.n_inner = gc.n_inner; g.L = gc.L;
    ProfScope ps(h, KC_GUIDE, ln.stream);
    HIPCHK(h, launch_guide(g, ln.stream));
    return 0;
}

// The step loop: every chunk through all steps, `nlanes` chunks at a time, each on its lane's stream - or, for jmid_net_eval, through
// that one step alone, e_theta to the chunk's staging rows.
int run_steps(jmid_ctx* h, const DenoiseCall& a, const CallPlan& cp, const CallIo& io) {
    const int E = a.E, A = a.A, K = a.K, T = a.T, lanes = cp.nlanes, nchunks = (int)cp.chunk_sizes.size(), n_steps = (int)h->beta.size();
    const size_t M = (size_t)E * K * A * T, tok = (size_t)K * A * T;       // tok: tokens per episode
    const bool one = a.single_step >= 0;
    const int i0 = one ? a.single_step : 0, i1 = one ? i0 + 1 : n_steps;
    // Opt-in (jmid_set_tuning "graph" = 1) for one-chunk calls: the whole denoise loop - n_steps x ~28 dependent launches on
    // workspace buffers only - is captured into a hipGraph the second time a shape is seen and replayed afterwards: one
    // graph launch instead of ~1400 kernel launches per call, bit-identical.  Measured on MI355X / ROCm 7.2
    // (tools/graph_latency.py): it does not pay - the GPU-side time is the same chain of kernels (a kernel boundary costs
    // the same inside a graph) and the replay itself is slower than the eager launches that run ahead of the GPU: one
    // scene 13.51 vs 13.08 ms per call, 4 scenes 28.40 vs 28.29, 8 scenes equal.  Off by default.
    // Inputs / outputs (copies, hyper-net GEMM, integrator) stay outside the graph.
    jmid_ctx::LoopGraph* lg = nullptr;
    bool capturing = false;
    if (a.single_step < 0 && lanes == 1 && nchunks == 1 && !h->prof_mask && !a.z && !h->ddpm && h->tune.graph == 1 &&
        h->tune.bystander_lds == 0 && !a.guide) {      // (a guided call's launches depend on its weights: never captured)
        const std::string key = std::to_string(E) + "," + std::to_string(A) + "," + std::to_string(K) + "," + std::to_string(T) +
                                "," + std::to_string(a.precision) + (cp.masked ? ",padded" : "");
        lg = &h->graphs[key];
        if (lg->exec && lg->arena != h->arena.p) {        // never true today (ensure_arena drops the graphs); cheap to keep
            hipGraphExecDestroy(lg->exec);
            lg->exec = nullptr;
        }
        if (lg->exec) {
            HIPCHK(h, hipGraphLaunch(lg->exec, h->stream));
            ++h->graph_replays;
        } else if (lg->warm) {
            HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            capturing = true;
        }
    }
    for (int c0 = 0; c0 < nchunks && !(lg && lg->exec); c0 += lanes) {
        // the steps of the chunks of this round are enqueued alternately so that all queues stay fed
        for (int i = i0; i < i1; ++i) {
            for (int l = 0; l < lanes; ++l) {
                if (c0 + l >= nchunks) break;
                const Lane& ln = cp.lanes[l];
                const size_t el = cp.chunk_start[c0 + l];
                float* xc = io.x_cur + el * tok * 2;
                const float* hc = io.hyp + el * A * h->hl.total;
                const float* zc = a.z ? a.z + ((size_t)i * M + el * tok) * 2 : nullptr;
                int rc = 0;
                if (cp.z_fill && h->p_noise[i]) {      // this step's draw for the chunk's episodes, on the chunk's own stream
                    rc = fill_noise(h, a.seeded->seed, h->noise_ids.get<unsigned>() + el, cp.chunk_sizes[c0 + l], tok * 2, i + 1, ln.z, nullptr, ln.stream);
                    zc = ln.z;
                }
                // layer 0's coefficient table of this chunk for all steps, ahead of its first step, on the chunk's own stream
                const StepPlan& pl = cp.plans[cp.chunk_plan[c0 + l]];
                if (!rc && i == 0 && pl.qkv0 && pl.cf.qkv0_steps > 1) rc = qkv0_build_table(h, pl, ln, hc, 0, n_steps);
                if (!rc && i == 0 && pl.tail_fold && pl.cf.tail_steps > 1) rc = tail_build_table(h, pl, ln, hc, 0, n_steps);
                // a guided call: the guide kernel sits between this step's update and the next step's embedding, so no seam is fused
                const bool fuse = h->tune.fuse_embed && !a.guide;
                if (!rc) rc = net_step(h, pl, ln, i, xc, hc, one ? io.stage + el * tok * 2 : nullptr, zc, fuse && i > i0,
                                        fuse && i + 1 < i1 ? i + 1 : -1,
                                        io.mask ? io.mask + el * mask_words_per_seq((int)tok) : nullptr);
                if (!rc && a.guide && a.guide->weights[i] > 0.0) rc = guide_chunk(h, a, io, ln, i, el, cp.chunk_sizes[c0 + l]);
                if (rc) {
                    if (capturing) {
                        hipGraph_t dead = nullptr;
                        (void)hipStreamEndCapture(h->stream, &dead);
                        if (dead) hipGraphDestroy(dead);
                    }
                    // the lanes share the one arena: what they already hold must have drained before the caller (the f32
                    // rerun, ensure_arena, jmid_destroy) touches it again on h->stream
                    sync_lanes(h);
                    return rc;
                }
            }
        }
    }
    if (capturing) {
        hipGraph_t graph = nullptr;
        HIPCHK(h, hipStreamEndCapture(h->stream, &graph));
        hipError_t ge = hipGraphInstantiate(&lg->exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (ge != hipSuccess) {
            lg->exec = nullptr;
            return fail(h, JMID_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ge));
        }
        lg->arena = h->arena.p;
        HIPCHK(h, hipGraphLaunch(lg->exec, h->stream));
        ++h->graph_replays;
    } else if (lg && !lg->exec) {
        lg->warm = true;
    }
    return 0;
}

// Join the lanes, integrate, hand the outputs over, and - unless the call is a stage of jmid_predict, which reads the range flag with
// its one download - bring the flag back.
int finish_call(jmid_ctx* h, const DenoiseCall& a, const CallPlan& cp, const CallIo& io) {
    const size_t R = (size_t)a.E * a.K * a.A, M = R * a.T;
    const hipMemcpyKind kout = a.mem == JMID_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (int l = 1; l < cp.nlanes; ++l) {
        HIPCHK(h, hipEventRecord(h->ev_join[l - 1], cp.lanes[l].stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[l - 1], 0));
    }
    // a padded call: quiet NaN in the padded agents' rows of what it returns - and, through the integrator, of the resident positions
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    if (const LossCall* lc = a.loss) {      // the staged e_theta against e, before the pad fill below touches the stage
        const LossReduceArgs ra{io.stage, io.e_dev, io.nag, io.loss_rows, io.loss, (int)R, a.A, a.T * 2};
        {
            ProfScope ps(h, KC_LOSS_REDUCE, h->stream);
            HIPCHK(h, launch_loss_reduce(ra, h->stream));
        }
        HIPCHK(h, hipMemcpyAsync(lc->loss_out, io.loss, 2 * sizeof(double), kout, h->stream));
        if (lc->row_out) HIPCHK(h, hipMemcpyAsync(lc->row_out, io.loss_rows, R * sizeof(double), kout, h->stream));
    }
    if (cp.masked) HIPCHK(h, launch_pad_fill(a.single_step >= 0 ? io.stage : io.x_cur, io.nag, a.E, a.K, a.A, a.T * 2, qnan, h->stream));
    if (a.single_step >= 0) {
        if (a.e_out) HIPCHK(h, hipMemcpyAsync(a.e_out, io.stage, M * 2 * sizeof(float), kout, h->stream));
    } else {
        if (a.vel_out) HIPCHK(h, hipMemcpyAsync(a.vel_out, io.x_cur, M * 2 * sizeof(float), kout, h->stream));
        if (a.guide && a.guide->guide_out)
            HIPCHK(h, hipMemcpyAsync(a.guide->guide_out, io.guide, (size_t)a.E * a.K * GDE_COLS * sizeof(float), kout, h->stream));
        if (a.p0) {      // integrated whenever p0 is given: the positions stay in the workspace for jmid_topk(pos = NULL)
            {
                ProfScope ps(h, KC_INTEGRATE, h->stream);
                const int n = (int)R * 2;
                hipLaunchKernelGGL(integrate_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, io.x_cur, a.p0,
                                   io.stage, (int)R, a.T, a.A, a.K * a.A, a.dt);
                HIPCHK(h, hipGetLastError());
            }
            h->last_pos = io.stage;
            h->last_pos_dims[0] = a.E; h->last_pos_dims[1] = a.A; h->last_pos_dims[2] = a.K; h->last_pos_dims[3] = a.T;
            if (a.pos_out) HIPCHK(h, hipMemcpyAsync(a.pos_out, io.stage, M * 2 * sizeof(float), kout, h->stream));
        }
    }
    if (a.chained) return 0;       // (no caller-stream ordering either)
    if (int rc = order_out(h, a.mem)) return rc;
    int flag = 0;      // an activation outside the fp16 range poisons the split operands: report it instead of returning garbage
    if (cp.mode.split) HIPCHK(h, hipMemcpyAsync(&flag, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (cp.mode.split || a.mem == JMID_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
    return flag ? flagged_call(h, flag) : 0;
}

int run_network(jmid_ctx* h, DenoiseCall a) {
    CallMode mode;
    if (int rc = check_call(h, a, &mode)) return rc;
    CallPlan cp = plan_call(h, a, mode);
    HIPCHK(h, hipSetDevice(h->device));
    if (!a.chained)
        if (int rc = order_in(h, a.mem)) return rc;
    CallIo io;
    if (int rc = fill_workspace(h, a, cp, io)) return rc;
    if (int rc = run_steps(h, a, cp, io)) return rc;
    return finish_call(h, a, cp, io);
}

// A call whose range flag came back set.  Bit 1 (gemm_small.hpp, OUT_LNX): a workgroup gave up waiting for a partner - nothing to do with
// the arithmetic: the handle drops that kernel for good and the caller repeats the call in the SAME precision (JMID_ETIMEOUT).  Otherwise
// bit 0: an activation left the fp16 range (JMID_ERANGE: repeat in JMID_PREC_F32).  Either way the outputs are undefined.
int flagged_call(jmid_ctx* h, int flag) {
    h->last_pos = nullptr;     // the integrated positions are poisoned too: jmid_topk(pos = NULL) must not rank them
    if (flag & 2) {
        h->lnx_off = true;
        ++h->lnx_timeouts;
        return fail(h, JMID_ETIMEOUT, "a workgroup of a one-launch GEMM + LayerNorm gave up waiting for its partners (not all workgroups of the launch "
                                      "were resident): this handle now runs the unfused kernels - repeat the call in the same precision");
    }
    ++h->erange_calls;
    return fail(h, JMID_ERANGE, "an activation left the fp16 range in JMID_PREC_F16X3 / F16X2 / F16MX: rerun with JMID_PREC_F32");
}

#ifdef JMID_DIAGNOSTICS
// The tail of a step in JMID_PREC_F32 on ln.X, launch for launch as net_step runs it: concat3, concat4 (ConcatSquash epilogues), then
// the output stage
int f32_tail(jmid_ctx* h, const StepPlan& p, const Lane& ln, int step_idx, float* x_chunk, const float* hyp_chunk, float* e_out,
             const float* z_chunk, int next_step) {
    const int M = p.M, d = h->d;
    const float* thyp = p.thyp(step_idx);
    GemmArgs g = gemm_args(p.rm, M, ln.X, h->wt.concat3, ln.Y3, h->dmid, d);
    g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total; g.goff = h->hl.g3; g.boff = h->hl.b3;
    if (int rc = run_gemm<EPI_CSL>(h, ln.stream, KC_GEMM_TAIL, g)) return rc;
    g = gemm_args(p.rm, M, ln.Y3, h->wt.concat4, ln.Y4, h->dlow, h->dmid);
    g.hyp = hyp_chunk; g.thyp = thyp; g.hyp_ld = h->hl.total; g.goff = h->hl.g4; g.boff = h->hl.b4;
    if (int rc = run_gemm<EPI_CSL>(h, ln.stream, KC_GEMM_TAIL, g)) return rc;
    return output_stage(h, p, ln, step_idx, x_chunk, hyp_chunk, e_out, z_chunk, next_step);
}

// jmid_dbg_qkv0 and jmid_dbg_tail: one piece of step `step` as a step of a one-chunk call on an idle handle runs it, on host buffers.
// tail = false: the embedding of x [M, 2] and layer 0's Q / K / V^T planes (the "qkv0" knob decides how), read back as fp32 [M, 3 d].
// tail = true: the tail alone on X [M, d] (fp32, split here into the planes the mode's concat3 reads: X_hi, and X_lo in F16X3) - folded,
// or the two GEMMs + the output kernel with "tail_fold" = 1 -> e [M, 2]; JMID_PREC_F32: the fp32 GEMMs + the output kernel on X itself.
int dbg_step(jmid_ctx* h, bool tail, int E, int A, int K, int T, const float* in, const float* hyp, int hyp_width, int step, int precision,
             float* out, float* thyp_row) {
    const std::string who = tail ? "jmid_dbg_tail" : "jmid_dbg_qkv0";
    CallMode mode;
    if (int rc = check_ready(h)) return rc;
    if (!in || !hyp || !out || E <= 0 || A <= 0 || K <= 0 || T <= 0 || T > kPeMaxLen) return fail(h, JMID_EINVAL, who + ": bad arguments");
    if (hyp_width != h->hl.total) return fail(h, JMID_EINVAL, who + ": hyp rows must be " + std::to_string(h->hl.total) + " wide");
    if (!call_mode(precision, &mode) || (!tail && (!mode.split || h->net_kind != JMID_NET_JMID)))
        return fail(h, JMID_EINVAL, who + (tail ? ": bad precision" : ": JMID in a split-fp16 mode only"));
    if (step < 0 || step >= (int)h->beta.size()) return fail(h, JMID_EINVAL, who + ": step outside the step table");
    HIPCHK(h, hipSetDevice(h->device));
    h->last_pos = nullptr;
    const size_t M = (size_t)E * K * A * T, EA = (size_t)E * A;
    const int d = h->d, in_w = tail ? d : 2, out_w = tail ? 2 : 3 * d;
    const StepPlan p = plan_step(h, E, A, K, T, mode, CallFacts{});      // (an idle handle: nothing else in flight, one launch, the table of one step)
    const size_t qkv0_rows = !tail && p.qkv0 ? EA * 3 : 0, tail_rows = tail && p.tail_fold ? EA : 0;
    float *in_d, *hyp_d, *out_d;
    const auto io = [&](char* base) {      // base null: the size only
        Carver c(base);
        in_d = c.take(M * in_w);
        hyp_d = c.take(EA * h->hl.total);
        out_d = c.take(M * out_w);
        return c.off;
    };
    const size_t io_off = io(nullptr);
    if (int rc = ensure_arena(h, io_off + step_ws_floats(h, M, mode, p.sg, 1, nullptr, nullptr, qkv0_rows, tail_rows), who.c_str())) return rc;
    io(h->arena.p);
    Lane ln{};
    ln.stream = h->stream;
    step_ws_floats(h, M, mode, p.sg, 1, &ln, h->arena.p + io_off, qkv0_rows, tail_rows);
    HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), h->stream));
    if (!tail) {
        HIPCHK(h, hipMemsetAsync(ln.Vth, 0, ln.vt_elems * sizeof(half_t), h->stream));
        HIPCHK(h, hipMemsetAsync(ln.Vtl, 0, ln.vt_elems * sizeof(half_t), h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(in_d, in, M * in_w * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(hyp_d, hyp, EA * h->hl.total * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (tail && !mode.split) {
        HIPCHK(h, hipMemcpyAsync(ln.X, in_d, M * d * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        if (int rc = f32_tail(h, p, ln, step, nullptr, hyp_d, out_d, nullptr, -1)) return rc;
    } else if (tail) {
        // (the planes' padding rows up to the next multiple of 128 only ever feed discarded output rows of the GEMM path, but must be finite)
        HIPCHK(h, hipMemsetAsync(ln.Xh, 0, blk_plane_elems(M, d) * sizeof(half_t), h->stream));
        HIPCHK(h, hipMemsetAsync(ln.Xl, 0, blk_plane_elems(M, d) * sizeof(half_t), h->stream));
        hipLaunchKernelGGL(tail_split_rows_kernel, dim3(512), dim3(256), 0, h->stream, in_d, ln.Xh, mode.x2 ? nullptr : ln.Xl, (int)M, d);
        HIPCHK(h, hipGetLastError());
        if (int rc = net_tail(h, p, ln, step, nullptr, hyp_d, out_d, nullptr, -1)) return rc;
    } else {
        if (int rc = run_embed(h, p, ln, in_d, hyp_d, p.thyp(step))) return rc;
        if (int rc = qkv_planes(h, p, ln, 0, step, in_d, hyp_d)) return rc;
        const LoImages im = lo_images(p, ln, d);
        QkvReadArgs ra{ln.Qh, ln.Ql, ln.Kh, ln.Kl, ln.Vth, ln.Vtl, im.q8l, im.k8l, out_d, M, d, p.hd, p.sg.S, p.sg.Spad, mode.x2,
                       p.att_scale * 1.4426950408889634f};
        hipLaunchKernelGGL(qkv_planes_read_kernel, dim3(512), dim3(256), 0, h->stream, ra);
        HIPCHK(h, hipGetLastError());
    }
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, out_d, M * out_w * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (thyp_row)
        HIPCHK(h, hipMemcpyAsync(thyp_row, p.thyp(step), h->hl.total * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return flag ? flagged_call(h, flag) : 0;
}

// jmid_dbg_seam: what net_step runs after the last layer of step `step` - the tail, the sampler update of x and, with next_step >= 0,
// the embedding of the updated x for step `next_step` - as the plan of a one-chunk call of that shape on an idle handle says, in the
// launches that plan says (net_tail in the split-fp16 modes; the two EPI_CSL GEMMs + output_stage in F32), all four modes, JMID and
// iMID, DDIM or DDPM as the handle's step table is.  X [M, d] is split as dbg_step splits it.  The hyper rows come from the call's own
// hyper GEMM on ctx (fill_workspace's launch), or are given.  The embedding's buffers are read back as two fp32 arrays after the
// launch; before it, every one of them that is not an input of the tail holds JMID_DBG_SEAM_FILL bytes (the others hold X as split).
// embed_only: run_embed alone on x at `step` (a call's first step), read back the same way.
int dbg_seam(jmid_ctx* h, int E, int A, int K, int T, const float* X, const float* x, const float* z, const float* ctx, const float* hyp,
             int hyp_width, int step, int next_step, int precision, int embed_only, float* x_next, float* hi, float* lo, float* hyp_out,
             float* thyp_rows, float* coef, int* plan) {
    const std::string who = "jmid_dbg_seam";
    CallMode mode;
    if (int rc = check_ready(h)) return rc;
    if ((!X && !embed_only) || !x || !x_next || !hi || !lo || !plan || (!ctx == !hyp) || E <= 0 || A <= 0 || K <= 0 || T <= 0 || T > kPeMaxLen)
        return fail(h, JMID_EINVAL, who + ": bad arguments");
    if (hyp && hyp_width != h->hl.total) return fail(h, JMID_EINVAL, who + ": hyp rows must be " + std::to_string(h->hl.total) + " wide");
    if (!call_mode(precision, &mode)) return fail(h, JMID_EINVAL, who + ": bad precision");
    if (mode.split && !h->weights_in_half_range) return fail(h, JMID_ERANGE, who + ": a weight exceeds the fp16 range");
    const int n_steps = (int)h->beta.size();
    if (step < 0 || step >= n_steps || next_step < -1 || next_step >= n_steps) return fail(h, JMID_EINVAL, who + ": step outside the step table");
    HIPCHK(h, hipSetDevice(h->device));
    h->last_pos = nullptr;
    const size_t M = (size_t)E * K * A * T, EA = (size_t)E * A;
    const int d = h->d, width = h->hl.total;
    const StepPlan p = plan_step(h, E, A, K, T, mode, CallFacts{});      // (an idle handle: nothing else in flight, one launch, the table of one step)
    const size_t tail_rows = !embed_only && p.tail_fold ? EA : 0;
    float *X_d, *x_d, *z_d, *ctx_d, *hyp_d, *hi_d, *lo_d;
    const auto io = [&](char* base) {      // base null: the size only
        Carver c(base);
        X_d = c.take(M * d);
        x_d = c.take(M * 2);
        z_d = c.take(M * 2);
        ctx_d = c.take(EA * h->ctx_dim);
        hyp_d = c.take(EA * width);
        hi_d = c.take(M * d);
        lo_d = c.take(M * d);
        return c.off;
    };
    const size_t io_off = io(nullptr);
    if (int rc = ensure_arena(h, io_off + step_ws_floats(h, M, mode, p.sg, 1, nullptr, nullptr, 0, tail_rows), who.c_str())) return rc;
    io(h->arena.p);
    Lane ln{};
    ln.stream = h->stream;
    step_ws_floats(h, M, mode, p.sg, 1, &ln, h->arena.p + io_off, 0, tail_rows);
    hipStream_t st = h->stream;
    const size_t plane_bytes = blk_plane_elems(M, d) * sizeof(half_t);
    if (mode.split) HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), st));
    HIPCHK(h, hipMemcpyAsync(x_d, x, M * 2 * sizeof(float), hipMemcpyHostToDevice, st));
    if (z) HIPCHK(h, hipMemcpyAsync(z_d, z, M * 2 * sizeof(float), hipMemcpyHostToDevice, st));
    if (ctx) {      // the ctx part of the four hyper nets as a call makes it (fill_workspace)
        HIPCHK(h, hipMemcpyAsync(ctx_d, ctx, EA * h->ctx_dim * sizeof(float), hipMemcpyHostToDevice, st));
        GemmArgs g{};
        g.A = ctx_d; g.lda = h->ctx_dim; g.W = h->Whyp; g.ldw = h->ctx_dim; g.bias = h->bhyp; g.C = hyp_d;
        g.ldc = width; g.M = (int)EA; g.N = width; g.K = h->ctx_dim;
        if (int rc = run_gemm<EPI_BIAS>(h, st, KC_HYPER, g)) return rc;
    } else {
        HIPCHK(h, hipMemcpyAsync(hyp_d, hyp, EA * width * sizeof(float), hipMemcpyHostToDevice, st));
    }
    int kernel;
    if (embed_only) {
        if (mode.split) {
            HIPCHK(h, hipMemsetAsync(ln.Xh, JMID_DBG_SEAM_FILL, plane_bytes, st));
            HIPCHK(h, hipMemsetAsync(ln.Xl, JMID_DBG_SEAM_FILL, plane_bytes, st));
        } else {
            HIPCHK(h, hipMemsetAsync(ln.X, JMID_DBG_SEAM_FILL, M * d * sizeof(float), st));
        }
        if (int rc = run_embed(h, p, ln, x_d, hyp_d, p.thyp(step))) return rc;
        kernel = JMID_DBG_SEAM_EMBED;
    } else if (mode.split) {
        HIPCHK(h, hipMemcpyAsync(X_d, X, M * d * sizeof(float), hipMemcpyHostToDevice, st));
        // (the planes' padding rows up to the next multiple of 128 only ever feed discarded output rows of the GEMM path, but must be finite)
        HIPCHK(h, hipMemsetAsync(ln.Xh, 0, plane_bytes, st));
        HIPCHK(h, hipMemsetAsync(ln.Xl, mode.x2 ? JMID_DBG_SEAM_FILL : 0, plane_bytes, st));      // F16X2 / F16MX: the tail reads X_hi only
        hipLaunchKernelGGL(tail_split_rows_kernel, dim3(512), dim3(256), 0, st, X_d, ln.Xh, mode.x2 ? nullptr : ln.Xl, (int)M, d);
        HIPCHK(h, hipGetLastError());
        if (int rc = net_tail(h, p, ln, step, x_d, hyp_d, nullptr, z ? z_d : nullptr, next_step)) return rc;
        kernel = p.tail_fold ? (p.out_tpw ? JMID_DBG_SEAM_FOLD_TRAJ : JMID_DBG_SEAM_FOLD) : (p.out_tpw ? JMID_DBG_SEAM_OUT_TRAJ : JMID_DBG_SEAM_OUT);
    } else {
        HIPCHK(h, hipMemcpyAsync(ln.X, X, M * d * sizeof(float), hipMemcpyHostToDevice, st));
        if (int rc = f32_tail(h, p, ln, step, x_d, hyp_d, nullptr, z ? z_d : nullptr, next_step)) return rc;
        kernel = p.out_tpw ? JMID_DBG_SEAM_OUT_TRAJ : JMID_DBG_SEAM_OUT;
    }
    // the embedding's buffers as the mode stores them -> hi / lo
    if (!mode.split) {
        HIPCHK(h, hipMemcpyAsync(hi_d, ln.X, M * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemsetAsync(lo_d, 0, M * d * sizeof(float), st));
    } else {
        if (p.mxv2) hipLaunchKernelGGL(merge_planes_lo8_kernel, dim3(512), dim3(256), 0, st, ln.Xh, reinterpret_cast<unsigned char*>(ln.Xl), hi_d, (int)M, lo_d);
        else hipLaunchKernelGGL(merge_planes_kernel, dim3(512), dim3(256), 0, st, ln.Xh, ln.Xl, hi_d, (int)M, d, lo_d);
        HIPCHK(h, hipGetLastError());
    }
    int flag = 0;
    if (mode.split) HIPCHK(h, hipMemcpyAsync(&flag, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(x_next, x_d, M * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hi, hi_d, M * d * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(lo, lo_d, M * d * sizeof(float), hipMemcpyDeviceToHost, st));
    if (hyp_out) HIPCHK(h, hipMemcpyAsync(hyp_out, hyp_d, EA * width * sizeof(float), hipMemcpyDeviceToHost, st));
    if (thyp_rows) {
        HIPCHK(h, hipMemcpyAsync(thyp_rows, p.thyp(step), width * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(thyp_rows + width, p.thyp(next_step >= 0 ? next_step : step), width * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    if (coef) {
        const float v[JMID_DBG_SEAM_COEF_WORDS] = {h->c_e[step], h->c_x[step], h->n_x[step], h->n_e[step],
                                                   h->ddpm ? h->p_c0[step] : 0.f, h->ddpm ? h->p_c1[step] : 0.f, h->ddpm ? h->p_sigma[step] : 0.f,
                                                   h->ddpm && h->p_noise[step] ? 1.f : 0.f};
        for (int i = 0; i < JMID_DBG_SEAM_COEF_WORDS; ++i) coef[i] = v[i];
    }
    const int words[JMID_DBG_SEAM_PLAN_WORDS] = {kernel, p.out_tpw, !mode.split ? 0 : p.mxv2 ? 2 : 1, h->ddpm ? 1 : 0,
                                                 !embed_only && next_step >= 0, p.tail_fold, flag};
    for (int i = 0; i < JMID_DBG_SEAM_PLAN_WORDS; ++i) plan[i] = words[i];
    return flag ? flagged_call(h, flag) : 0;
}

// jmid_dbg_layer: encoder layer `layer` of one step, launch for launch as net_step runs it in a one-chunk call on an idle handle (the
// facts - the split-KV factor included - are plan_call's for that shape), on X [M, d] given in fp32 and split here into the planes the
// mode's layer reads.  After every stage its planes are copied out on the same stream as two fp32 arrays: hi and lo, M x
// JMID_DBG_LAYER_WIDTH(d, ff) floats each, hold stage s as the row-major [M, width of the stage] block at M x off[s].
// The stages and plan [JMID_DBG_LAYER_PLAN_WORDS]: include/jmid_hip.h.
int dbg_layer(jmid_ctx* h, int E, int A, int K, int T, int layer, int precision, const float* X, const int32_t* n_agents, int last,
              float* hi, float* lo, int* plan) {
    const std::string who = "jmid_dbg_layer";
    CallMode mode;
    if (int rc = check_ready(h)) return rc;
    if (!X || !hi || !lo || !plan || E <= 0 || A <= 0 || K <= 0 || T <= 0 || T > kPeMaxLen) return fail(h, JMID_EINVAL, who + ": bad arguments");
    if (!call_mode(precision, &mode)) return fail(h, JMID_EINVAL, who + ": bad precision");
    if (layer < 0 || layer >= h->tf_layer) return fail(h, JMID_EINVAL, who + ": layer outside the encoder");
    if (mode.split && !h->weights_in_half_range) return fail(h, JMID_ERANGE, who + ": a weight exceeds the fp16 range");
    if (n_agents) {
        if (int rc = check_n_agents(h, who.c_str(), n_agents, E, A)) return rc;
        if (h->net_kind == JMID_NET_JMID && mode.split && !attn_masked_built(plan_attn(h->d / h->nhead, h->tune), mode.x2 != 0))
            return fail(h, JMID_EINVAL, who + ": the attention kernel these knobs select has no masked form");
    }
    HIPCHK(h, hipSetDevice(h->device));
    h->last_pos = nullptr;
    DenoiseCall call{};
    call.E = E; call.A = A; call.K = K; call.T = T; call.precision = precision; call.mem = JMID_MEM_HOST;
    call.single_step = 0; call.n_agents = n_agents; call.who = "jmid_dbg_layer";
    CallFacts cf = plan_call(h, call, mode).facts;      // (the split-KV factor: the call's shape, mode and knob only)
    cf.small_now = 1;                                   // one chunk on an idle handle
    cf.one_chunk = h->tune.graph != 1;
    const StepPlan p = plan_step(h, E, A, K, T, mode, cf, n_agents != nullptr);
    const bool split = mode.split, joint = p.joint;
    const int M = p.M, d = h->d, ff = h->ff, S = p.sg.S, nseq = p.sg.nseq, hd = p.hd;
    const size_t Mz = (size_t)M, width = 7 * (size_t)d + ff;
    const size_t off[6] = {0, (size_t)d, 4 * (size_t)d, 5 * (size_t)d, 6 * (size_t)d, 6 * (size_t)d + ff};
    const bool mask_words = n_agents && joint;
    float *in_d, *hi_d, *lo_d;
    unsigned* mask_d;
    const auto io = [&](char* base) {      // base null: the size only
        Carver c(base);
        in_d = c.take(Mz * d);
        hi_d = c.take(Mz * width);
        lo_d = c.take(Mz * width);
        mask_d = mask_words ? reinterpret_cast<unsigned*>(c.take((size_t)E * mask_words_per_seq(S))) : nullptr;
        return c.off;
    };
    const size_t io_off = io(nullptr);
    if (int rc = ensure_arena(h, io_off + step_ws_floats(h, Mz, mode, p.sg, cf.attn_nsplit, nullptr, nullptr, 0, 0), who.c_str())) return rc;
    io(h->arena.p);
    Lane ln{};
    ln.stream = h->stream;
    step_ws_floats(h, Mz, mode, p.sg, cf.attn_nsplit, &ln, h->arena.p + io_off, 0, 0);
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemsetAsync(lo_d, 0, Mz * width * sizeof(float), st));
    HIPCHK(h, hipMemcpyAsync(in_d, X, Mz * d * sizeof(float), hipMemcpyHostToDevice, st));
    if (mask_words) {
        if (int rc = h->nag.upload(h, n_agents, E, who.c_str())) return rc;
        HIPCHK(h, launch_mask_words(h->nag.get<int>(), mask_d, E, A, T, S, st));
    }
    unsigned char* Xl8 = p.mxv2 ? reinterpret_cast<unsigned char*>(ln.Xl) : nullptr;
    // a stage's planes -> hi_d / lo_d at its offset
    const auto out_hi = [&](int s) { return hi_d + Mz * off[s]; };
    const auto out_lo = [&](int s) { return lo_d + Mz * off[s]; };
    const auto copy_f32 = [&](int s, const float* src, size_t w) {
        return hipMemcpyAsync(out_hi(s), src, Mz * w * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    const auto read_x = [&](int s, bool lo_written) {      // the residual stream
        if (!split) return copy_f32(s, ln.X, d);
        if (p.mxv2) hipLaunchKernelGGL(merge_planes_lo8_kernel, dim3(512), dim3(256), 0, st, ln.Xh, lo_written ? Xl8 : nullptr, out_hi(s), M, out_lo(s));
        else hipLaunchKernelGGL(merge_planes_kernel, dim3(512), dim3(256), 0, st, ln.Xh, lo_written ? ln.Xl : nullptr, out_hi(s), M, d, out_lo(s));
        return hipGetLastError();
    };
    const auto read_planes = [&](int s, const half_t* ph, const half_t* pl, int w) {
        hipLaunchKernelGGL(merge_planes_kernel, dim3(512), dim3(256), 0, st, ph, pl, out_hi(s), M, w, out_lo(s));
        return hipGetLastError();
    };
    int stages = 0;
    // ---- stage 0: X as the layer reads it
    if (!split) {
        HIPCHK(h, hipMemcpyAsync(ln.X, in_d, Mz * d * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), st));
        HIPCHK(h, hipMemsetAsync(ln.ln_xchg, 0, kLnxWords * sizeof(unsigned), st));
        // (the planes' padding rows up to the next multiple of 128 only ever feed discarded output rows, but must be finite)
        half_t* const planes[6] = {ln.Xh, ln.Xl, ln.Ah, ln.Al, ln.H1h, ln.H1l};
        const int plane_w[6] = {d, d, d, d, ff, ff};
        for (int i = 0; i < 6; ++i) HIPCHK(h, hipMemsetAsync(planes[i], 0, blk_plane_elems(Mz, plane_w[i]) * sizeof(half_t), st));
        if (ln.Vth) {
            HIPCHK(h, hipMemsetAsync(ln.Vth, 0, ln.vt_elems * sizeof(half_t), st));
            HIPCHK(h, hipMemsetAsync(ln.Vtl, 0, ln.vt_elems * sizeof(half_t), st));
        }
        if (p.mxv2) hipLaunchKernelGGL(split_planes_lo8_kernel, dim3(512), dim3(256), 0, st, in_d, ln.Xh, Xl8, M);
        else hipLaunchKernelGGL(split_planes_blocked_kernel, dim3(512), dim3(256), 0, st, in_d, ln.Xh, ln.Xl, M, d, h->range_flag, 1.0f);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, read_x(0, true));
    stages |= 1;
    const LayerW& w = h->wt.layers[layer];
    const RowMap& rm = p.rm;
    // ---- stages 1 and 2: Q / K / V and the attention on them (net_step)
    if (!split) {
        if (int rc = run_gemm<EPI_BIAS>(h, st, KC_GEMM_QKV, gemm_args(rm, M, ln.X, w.in_proj, ln.QKV, 3 * d, d))) return rc;
        HIPCHK(h, copy_f32(1, ln.QKV, 3 * (size_t)d));
        AttnArgs aa{ln.QKV, ln.ATT, S, d, h->nhead, p.att_scale, nullptr, nullptr};
        aa.mask = p.attn.masked ? mask_d : nullptr;
        HIPCHK(h, launch_attn_f32(aa, nseq, hd, p.attn.pack, st));
        HIPCHK(h, copy_f32(2, ln.ATT, d));
        stages |= 6;
        if (int rc = run_gemm<EPI_BIAS>(h, st, KC_GEMM_OUT, gemm_args(rm, M, ln.ATT, w.out_proj, ln.Y, d, d))) return rc;
        if (int rc = run_add_ln(h, st, ln.X, ln.Y, w.norm1.gamma, w.norm1.beta, M, d)) return rc;
        HIPCHK(h, read_x(3, true));
        if (int rc = run_gemm<EPI_BIAS_RELU>(h, st, KC_GEMM_FF1, gemm_args(rm, M, ln.X, w.linear1, ln.H1, ff, d))) return rc;
        HIPCHK(h, copy_f32(4, ln.H1, ff));
        if (int rc = run_gemm<EPI_BIAS>(h, st, KC_GEMM_FF2, gemm_args(rm, M, ln.H1, w.linear2, ln.Y, d, ff))) return rc;
        if (int rc = run_add_ln(h, st, ln.X, ln.Y, w.norm2.gamma, w.norm2.beta, M, d)) return rc;
        HIPCHK(h, read_x(5, true));
        stages |= 56;
    } else {
        GemmHArgs g{};
        if (joint) {
            if (int rc = in_proj_planes(h, p, ln, layer)) return rc;
            const LoImages im = lo_images(p, ln, d);
            QkvReadArgs ra{ln.Qh, ln.Ql, ln.Kh, ln.Kl, ln.Vth, ln.Vtl, im.q8l, im.k8l, out_hi(1), Mz, d, hd, S, p.sg.Spad, mode.x2,
                           p.att_scale * 1.4426950408889634f, out_lo(1)};
            hipLaunchKernelGGL(qkv_planes_read_kernel, dim3(512), dim3(256), 0, st, ra);
            HIPCHK(h, hipGetLastError());
            AttnHArgs aa{ln.Qh, ln.Ql, ln.Kh, ln.Kl, ln.Vth, ln.Vtl, ln.Ah, ln.Al, S, p.sg.Spad, d, h->nhead,
                         p.att_scale, h->range_flag, p.cf.attn_nsplit, ln.Opart, ln.MLpart, p.mode.x2, im.k8h, im.k8l, im.q8l};
            aa.skip_combine = p.out_proj.merge;
            HIPCHK(h, launch_attn_f16x3(aa, nseq, hd, p.attn, st, p.attn.masked ? mask_d : nullptr));
            if (!p.out_proj.merge) {
                HIPCHK(h, read_planes(2, ln.Ah, mode.x2 ? nullptr : ln.Al, d));      // (F16X2 / F16MX: O_lo is not written)
                stages |= 4;
            }
        } else {
            g = gemm_h_args(p.mode, rm, M, ln.Xh, ln.Xl, w.in_proj, 3 * d, d);
            g.C = ln.QKV; g.ldc = 3 * d;
            if (int rc = (run_gemm_h<EPI_BIAS, OUT_F32>(h, st, KC_GEMM_QKV, g, p.in_proj))) return rc;
            HIPCHK(h, copy_f32(1, ln.QKV, 3 * (size_t)d));
            AttnArgs aa{ln.QKV, nullptr, S, d, h->nhead, p.att_scale, ln.Ah, ln.Al};
            HIPCHK(h, launch_attn_f32(aa, nseq, hd, p.attn.pack, st));
            HIPCHK(h, read_planes(2, ln.Ah, ln.Al, d));
            stages |= 4;
        }
        stages |= 2;
        // ---- stage 3: out_proj + residual + norm1
        if (int rc = residual_block(h, p, p.out_proj, ln, ln.Ah, ln.Al, d, w.out_proj, w.norm1, KC_GEMM_OUT, false)) return rc;
        HIPCHK(h, read_x(3, true));
        // ---- stage 4: linear1 + ReLU
        g = gemm_h_args(p.mode, rm, M, ln.Xh, ln.Xl, w.linear1, ff, d);
        g.Chi = ln.H1h; g.Clo = ln.H1l; g.ldc = ff;
        if (int rc = (run_gemm_h<EPI_BIAS_RELU, OUT_SPLIT>(h, st, KC_GEMM_FF1, g, p.linear1))) return rc;
        HIPCHK(h, read_planes(4, ln.H1h, mode.x2 ? nullptr : ln.H1l, ff));      // (F16X2 / F16MX: the consumer GEMM takes A_hi only)
        // ---- stage 5: linear2 + residual + norm2
        if (int rc = residual_block(h, p, p.linear2, ln, ln.H1h, ln.H1l, ff, w.linear2, w.norm2, KC_GEMM_FF2, last != 0)) return rc;
        // (last in F16X2 / F16MX: nothing reads the lo plane and most paths do not write it - GEMM + add_ln in F16X2 still does -:
        //  it is reported as zero, the plane concat3 reads is the hi plane alone)
        HIPCHK(h, read_x(5, !(last && mode.x2)));
        stages |= 56;
    }
    // the arithmetic of a residual block's GEMM (GemmMode): the row-tile kernels take the fp8 correction wherever the weight has its image
    const auto block_mode = [&](const ResidualPlan& rp, const LinearW& lin) {
        if (rp.path == RB_GEMM_LN2 || rp.path == RB_LNX_SMALL) return (int)GM_MX;
        if (rp.path == RB_GEMM_LN) return (int)(mode.mx && lin.w8 ? GM_MX : mode.x2 ? GM_X2 : GM_X3);
        return (int)rp.gemm.mode;
    };
    int flag = 0;
    if (split) HIPCHK(h, hipMemcpyAsync(&flag, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hi, hi_d, Mz * width * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(lo, lo_d, Mz * width * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int words[JMID_DBG_LAYER_PLAN_WORDS] = {
        stages, split ? p.in_proj.mode : -1, split ? p.in_proj.shape : -1, split ? p.in_proj.flags : 0,
        split ? p.linear1.mode : -1, split ? p.linear1.shape : -1, split ? p.linear1.flags : 0,
        split ? p.out_proj.path : -1, split ? p.out_proj.ln_rows : 0, split ? (int)p.out_proj.gemm.shape : -1,
        split ? p.linear2.path : -1, split ? p.linear2.ln_rows : 0, split ? (int)p.linear2.gemm.shape : -1,
        p.vt_direct, p.k8, p.q8l, p.cf.attn_nsplit, p.attn.masked, p.out_proj.merge, p.mxv2, p.attn.dma, flag,
        split ? block_mode(p.out_proj, w.out_proj) : -1, split ? block_mode(p.linear2, w.linear2) : -1, p.attn.pack};
    for (int i = 0; i < JMID_DBG_LAYER_PLAN_WORDS; ++i) plan[i] = words[i];
    return flag ? flagged_call(h, flag) : 0;
}
#endif

int launch_episode_metrics(jmid_ctx* h, const float* pos, const float* gt, float* out, int E, int K, int A, int T) {
    ProfScope ps(h, KC_METRICS, h->stream);
    hipLaunchKernelGGL(episode_metrics_kernel, dim3(E), dim3(256), 0, h->stream, pos, gt, out, K, A, T);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // namespace jmid_host


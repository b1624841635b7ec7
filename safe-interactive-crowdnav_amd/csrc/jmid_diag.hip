// libjmid_hip.so -- jmid_dbg_* single-kernel entry points (diagnostics flavour only).
#include "jmid_ctx.hpp"
#include "jmid_launch.hpp"

#include <deque>

#ifdef JMID_DIAGNOSTICS
// ---------------------------------------------------------------------------------------------- diagnostics
// Single-op entry points used by the unit tests (host buffers only).

// What the entry points that launch start with: the mode of their `precision`, the device, the handle's range flag
static int dbg_open(jmid_ctx* h, int precision, CallMode* mode) {
    if (!call_mode(precision, mode)) return fail(h, JMID_EINVAL, "bad precision");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->range_flag) {
        HIPCHK(h, hipMalloc((void**)&h->range_flag, sizeof(int)));
        HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), h->stream));
    }
    return 0;
}

// The device temporaries of one jmid_dbg_* call: local owners, so every exit frees them.  take(): `bytes` of device memory holding
// `host`'s bytes (host null: uninitialised), or null with the error set
struct DbgTemps {
    jmid_ctx* h;
    const char* who;
    std::deque<Block> blocks;
    int rc = 0;                    // the first failure: the caller looks once, after its takes
    template <class T>
    T* take(size_t bytes, const void* host = nullptr) {
        if (rc) return nullptr;
        blocks.emplace_back();
        Block& b = blocks.back();
        if ((rc = b.reserve(h, bytes, who))) return nullptr;
        const hipError_t e = host ? hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
        if (e != hipSuccess) rc = fail(h, JMID_EHIP, std::string(who) + ": " + hipGetErrorString(e));
        return rc ? nullptr : b.as<T>();
    }
    template <class T>
    T* zeros(size_t bytes) {       // ... zero-filled, on the handle's stream
        T* p = take<T>(bytes);
        if (p && hipMemsetAsync(p, 0, bytes, h->stream) != hipSuccess) rc = fail(h, JMID_EHIP, std::string(who) + ": memset failed");
        return rc ? nullptr : p;
    }
};
// the bf8 image of W_lo (what make_w8 gives the weight registry), as a temporary
static unsigned char* dbg_w8(DbgTemps& t, const float* dW, int N, int K) {
    unsigned char* p = t.take<unsigned char>((size_t)N * K);
    if (p) t.rc = w8_image(t.h, dW, N, K, p);
    return t.rc ? nullptr : p;
}

// one array of a layout -> (byte offset from the block's base, bytes); an array the call does not have: (-1, 0)
template <class T>
static void put_arr(int64_t*& w, const Arr<T>& a, const char* base) {
    *w++ = a.n ? (const char*)a.p - base : -1;
    *w++ = (int64_t)a.bytes();
}

extern "C" {

// The chunk plan of a mode without the one-launch rule (JMID_PREC_F16X3)
int jmid_dbg_plan_chunks(int net_kind, int nhead, int lanes, int chunk_episodes, int E, int tokens_per_episode, int* sizes, int cap) {
    return jmid_dbg_plan_chunks_mode(net_kind, nhead, lanes, chunk_episodes, E, tokens_per_episode, JMID_PREC_F16X3, sizes, cap);
}

// ... in arithmetic mode `precision` (the plan of a small batch depends on it: at most 2 560 tokens stay ONE chunk in JMID_PREC_F16MX)
int jmid_dbg_plan_chunks_mode(int net_kind, int nhead, int lanes, int chunk_episodes, int E, int tokens_per_episode, int precision, int* sizes, int cap) {
    CallMode mode;
    if (E <= 0 || tokens_per_episode <= 0 || nhead <= 0 || !sizes || cap <= 0 || !call_mode(precision, &mode)) return JMID_EINVAL;
    jmid_ctx ctx;                      // host fields only: the planner reads net_kind, nhead, lanes, chunk_eps and the tuning (model dimensions at their defaults: d_model 512)
    ctx.net_kind = net_kind; ctx.nhead = nhead; ctx.lanes = lanes; ctx.chunk_eps = chunk_episodes;
    const std::vector<int> plan = plan_chunks(&ctx, mode, E, tokens_per_episode);
    for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) sizes[i] = plan[i];
    return (int)plan.size();
}

int jmid_dbg_gemm_plan(int mode, int epi, int out, int M, int N, int K, int small_now, int one_chunk, const int* knobs, int* plan) {
    if (mode < GM_X3 || mode > GM_MX || epi < EPI_BIAS || epi > EPI_CSL || (out != OUT_F32 && out != OUT_SPLIT && out != OUT_QKV && out != OUT_LNX) ||
        M <= 0 || N <= 0 || K <= 0 || !knobs || !plan || knobs[0] < 0 || knobs[0] > 8)
        return JMID_EINVAL;
    Tuning t;
    int Tuning::*const fields[JMID_DBG_GEMM_PLAN_KNOBS] = {&Tuning::gemm_h_variant, &Tuning::gemm_small, &Tuning::ln_rows, &Tuning::small_lnx, &Tuning::small_lnx2,
                                                           &Tuning::cus, &Tuning::vt_stage, &Tuning::csl_swap, &Tuning::h1_stage, &Tuning::gemm_pn,
                                                           &Tuning::small_qk, &Tuning::small_pn, &Tuning::gemm_ng};
    for (int i = 0; i < JMID_DBG_GEMM_PLAN_KNOBS; ++i) t.*fields[i] = knobs[i];
    CallFacts cf;
    cf.small_now = small_now;
    cf.one_chunk = one_chunk;
    const GemmPlan p = plan_gemm((GemmMode)mode, epi, out, M, N, K, cf, t);
    plan[0] = p.mode; plan[1] = p.shape; plan[2] = p.flags; plan[3] = p.group_tiles;
    plan[4] = gemm_shape_bm(p.shape); plan[5] = gemm_shape_bn(p.shape);
    plan[6] = plan_ln_rows(false, M, t); plan[7] = plan_ln_rows(true, M, t);
    return JMID_OK;
}

// chain_io and scene_arrays on a handle that lives on the stack (host fields only) and blocks of host memory: no HIP call
int jmid_dbg_chain_layout(int hist_len, int ctx_dim, int E, int A, int K, int T, int k, int N, int flags, int64_t* chain_dev, int64_t* chain_pin,
                          int64_t* scene) {
    const bool in_scene = flags & JMID_DBG_LAYOUT_SCENE, forecast = flags & JMID_DBG_LAYOUT_FORECAST, seeded = flags & JMID_DBG_LAYOUT_SEEDED,
               first = flags & JMID_DBG_LAYOUT_FIRST_INDEX, pos = flags & JMID_DBG_LAYOUT_POS, cv = flags & JMID_DBG_LAYOUT_CV;
    if (!chain_dev || !chain_pin || !scene || hist_len < 1 || ctx_dim < 2 || E < 1 || A < 1 || K < 1 || T < 1 || k < 1 || k > K || N < 1) return JMID_EINVAL;
    if (!in_scene && (forecast || seeded || first)) return JMID_EINVAL;      // what exists in scene mode only
    if (forecast ? !cv || pos : k == K && !pos) return JMID_EINVAL;          // a forecast needs the scene's cv and downloads no pos; k == K needs pos_out
    jmid_ctx ctx;
    ctx.hist_len = hist_len; ctx.ctx_dim = ctx_dim; ctx.H = ctx_dim / 2;
    jmid_ctx::SceneWs& sc = ctx.scene;
    const int horizon = cv ? T : 0;
    std::vector<char> sbuf(scene_arrays(E, N, hist_len, horizon, first, nullptr, nullptr));
    const size_t s_total = scene_arrays(E, N, hist_len, horizon, first, sbuf.data(), &sc.arr);
    sc.E = E; sc.N = N; sc.horizon = horizon;
    const SceneArrays& a = sc.arr;
    int64_t* w = scene;
    put_arr(w, a.grid.human_xy, sbuf.data()); put_arr(w, a.grid.robot_xy, sbuf.data()); put_arr(w, a.grid.pose_now, sbuf.data());
    put_arr(w, a.x, sbuf.data()); put_arr(w, a.x_st, sbuf.data()); put_arr(w, a.nbr_sum, sbuf.data()); put_arr(w, a.edge_mask, sbuf.data());
    put_arr(w, a.p0, sbuf.data()); put_arr(w, a.n_in, sbuf.data()); put_arr(w, a.in_cluster, sbuf.data()); put_arr(w, a.robot_in, sbuf.data());
    put_arr(w, a.cv, sbuf.data()); put_arr(w, a.first_index, sbuf.data());
    *w++ = (const char*)a.x.p - sbuf.data();                  // the grid block: the bytes in front of x
    *w++ = (const char*)a.n_in.p - sbuf.data(); *w++ = (int64_t)a.down_bytes; *w++ = (int64_t)s_total;
    float some = 0.f;
    double some_d = 0.0;
    const uint32_t id = 0;
    const SeedArgs sa{0, &id};
    ChainCall c{E, A, K, T, k, JMID_PREC_F32};
    c.scene = in_scene; c.forecast = forecast; c.padded = flags & JMID_DBG_LAYOUT_PADDED;
    if (seeded) c.seeded = &sa;
    else c.x_T = &some;
    if (flags & JMID_DBG_LAYOUT_BW) c.bw = &some;
    if (pos) c.pos_out = &some;
    if (forecast) c.forecasts_out = c.logw_out = &some_d;
    for (int pinned = 0; pinned < 2; ++pinned) {
        std::vector<char> buf(chain_io(&ctx, c, nullptr, nullptr, pinned));
        ChainIo io;
        const size_t total = chain_io(&ctx, c, buf.data(), &io, pinned);
        w = pinned ? chain_pin : chain_dev;
        put_arr(w, io.x_st, buf.data()); put_arr(w, io.nbr_sum, buf.data()); put_arr(w, io.edge_mask, buf.data()); put_arr(w, io.x_T, buf.data());
        put_arr(w, io.p0, buf.data()); put_arr(w, io.bw, buf.data()); put_arr(w, io.ctx, buf.data()); put_arr(w, io.flag, buf.data());
        put_arr(w, io.forecasts, buf.data()); put_arr(w, io.logw_d, buf.data()); put_arr(w, io.sel, buf.data()); put_arr(w, io.logw, buf.data());
        put_arr(w, io.pos, buf.data()); put_arr(w, io.first_index, buf.data());
        *w++ = (const char*)io.x_st.p - buf.data(); *w++ = (int64_t)io.up_bytes;
        *w++ = (const char*)io.flag.p - buf.data(); *w++ = (int64_t)io.down_bytes; *w++ = (int64_t)total;
    }
    return JMID_OK;
}

int jmid_dbg_gemm(jmid_handle_t h, int M, int N, int K, const float* A, const float* Wt, const float* bias, int relu,
                  int precision, float* C) {
    if (!h || !A || !Wt || !C) return JMID_EINVAL;
    CallMode mode;
    if (int rc = dbg_open(h, precision, &mode)) return rc;
    DbgTemps t{h, "jmid_dbg_gemm"};
    float* dA = t.take<float>((size_t)M * K * 4, A);
    float* dW = t.take<float>((size_t)N * K * 4, Wt);
    float* dC = t.take<float>((size_t)M * N * 4);
    float* dB = bias ? t.take<float>((size_t)N * 4, bias) : nullptr;
    if (t.rc) return t.rc;
    int rc = 0;
    if (precision == JMID_PREC_F32) {
        GemmArgs g{};
        g.A = dA; g.lda = K; g.W = dW; g.ldw = K; g.bias = dB; g.C = dC; g.ldc = N; g.M = M; g.N = N; g.K = K;
        rc = relu ? run_gemm<EPI_BIAS_RELU>(h, h->stream, KC_GEMM_QKV, g) : run_gemm<EPI_BIAS>(h, h->stream, KC_GEMM_QKV, g);
    } else {
        const size_t pa = blk_plane_elems(M, K) * 2, pw = blk_plane_elems(N, K) * 2;
        half_t *ah = t.zeros<half_t>(pa), *al = t.zeros<half_t>(pa), *wh = t.zeros<half_t>(pw), *wl = t.zeros<half_t>(pw);
        if (t.rc) return t.rc;
        hipLaunchKernelGGL(split_planes_blocked_kernel, dim3(512), dim3(256), 0, h->stream, dA, ah, al, M, K,
                           h->range_flag, 1.0f);
        hipLaunchKernelGGL(split_planes_blocked_kernel, dim3(512), dim3(256), 0, h->stream, dW, wh, wl, N, K,
                           h->range_flag, kWScale);
        GemmHArgs g{};
        g.Ahi = ah; g.Alo = al; g.Whi = wh; g.Wlo = wl; g.bias = dB; g.C = dC; g.ldc = N;
        g.M = M; g.N = N; g.K = K; g.x2 = mode.x2;
        if (mode.mx && N % 32 == 0 && K % 64 == 0)
            if (!(g.W8 = dbg_w8(t, dW, N, K))) return t.rc;
        // (an idle handle: nothing else in flight, one launch)
        const GemmPlan plan = plan_gemm(mode.gemm, relu ? EPI_BIAS_RELU : EPI_BIAS, OUT_F32, M, N, K, CallFacts{}, h->tune);
        rc = relu ? run_gemm_h<EPI_BIAS_RELU, OUT_F32>(h, h->stream, KC_GEMM_QKV, g, plan) : run_gemm_h<EPI_BIAS, OUT_F32>(h, h->stream, KC_GEMM_QKV, g, plan);
    }
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int jmid_dbg_attention(jmid_handle_t h, int nseq, int S, const float* QKV, int precision, float* OUT) {
    if (!h || !QKV || !OUT) return JMID_EINVAL;
    CallMode mode;
    if (int rc = dbg_open(h, precision, &mode)) return rc;
    const size_t Mt = (size_t)nseq * S;
    const int d = h->d, hd = h->d / h->nhead;
    DbgTemps t{h, "jmid_dbg_attention"};
    float* dQ = t.take<float>(Mt * 3 * d * 4, QKV);
    float* dO = t.take<float>(Mt * d * 4);
    if (t.rc) return t.rc;
    int rc = 0;
    if (precision == JMID_PREC_F32) {
        AttnArgs aa{dQ, dO, S, d, h->nhead, 1.0f / sqrtf((float)hd), nullptr, nullptr};
        ProfScope ps(h, KC_ATTN, h->stream);
        hipError_t e = launch_attn_f32(aa, nseq, hd, plan_attn(hd, h->tune).pack, h->stream);
        if (e != hipSuccess) rc = fail(h, JMID_EHIP, hipGetErrorString(e));
    } else {
        const int Spad = vt_spad(S);
        const size_t vt = (size_t)nseq * d * Spad;
        half_t* b[8];
        const size_t sz[8] = {Mt * d, Mt * d, Mt * d, Mt * d, vt, vt, blk_plane_elems(Mt, d), blk_plane_elems(Mt, d)};
        for (int i = 0; i < 8; ++i) b[i] = t.zeros<half_t>(sz[i] * sizeof(half_t));
        if (t.rc) return t.rc;
        hipLaunchKernelGGL(qkv_to_planes_kernel, dim3(512), dim3(256), 0, h->stream, dQ, b[0], b[1], b[2], b[3], b[4],
                           b[5], Mt, d, hd, S, Spad, 1.4426950408889634f / sqrtf((float)hd));
        int ns = 1;
        float *opart = nullptr, *mlpart = nullptr;
        if (hd == 128) ns = attn_pick_nsplit(((S + 127) / 128) * h->nhead * nseq, S);
        if (ns > 1) {
            opart = t.take<float>((size_t)ns * Mt * d * 4);
            mlpart = t.take<float>((size_t)ns * Mt * h->nhead * 2 * 4);
            if (t.rc) return t.rc;
        }
        AttnHArgs aa{b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], S, Spad, d, h->nhead, 1.0f / sqrtf((float)hd),
                     h->range_flag, ns, opart, mlpart, mode.x2};
        {
            ProfScope ps(h, KC_ATTN, h->stream);
            hipError_t e = launch_attn_f16x3(aa, nseq, hd, plan_attn(hd, h->tune), h->stream);
            if (e != hipSuccess) rc = fail(h, JMID_EHIP, hipGetErrorString(e));
        }
        hipLaunchKernelGGL(merge_planes_kernel, dim3(512), dim3(256), 0, h->stream, b[6], b[7], dO, (int)Mt, d, (float*)nullptr);
    }
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(OUT, dO, Mt * d * 4, hipMemcpyDeviceToHost));
    return 0;
}

int jmid_dbg_gemm_ln_mx(jmid_handle_t h, int M, int K, const float* A, const float* Wt, const float* bias, const float* gamma,
                        const float* beta, float* X, int fused) {
    // X <- LayerNorm(X + A . Wt^T + bias) in JMID_PREC_F16MX at d_model 512 with the second-generation kernels
    // (gemm_ln2_mx.hpp): fused = 1 the row-complete kernel, 0 the GEMM + add_ln2 pair.  X comes back as hi + bf8(lo).
    if (!h || !A || !Wt || !bias || !gamma || !beta || !X || M <= 0 || K % 64 != 0) return JMID_EINVAL;
    constexpr int N = GLN_BN;
    CallMode mode;
    if (int rc = dbg_open(h, JMID_PREC_F16MX, &mode)) return rc;
    DbgTemps t{h, "jmid_dbg_gemm_ln_mx"};
    float* dA = t.take<float>((size_t)M * K * 4, A);
    float* dW = t.take<float>((size_t)N * K * 4, Wt);
    float* dB = t.take<float>(N * 4, bias);
    float* dG = t.take<float>(N * 4, gamma);
    float* dT = t.take<float>(N * 4, beta);
    float* dX = t.take<float>((size_t)M * N * 4, X);
    float* dY = t.zeros<float>((size_t)(M + 63) / 64 * 64 * N * 4);
    const size_t pa = blk_plane_elems(M, K) * 2, pw = blk_plane_elems(N, K) * 2, px = blk_plane_elems(M, N) * 2;
    half_t *ah = t.zeros<half_t>(pa), *al = t.zeros<half_t>(pa), *wh = t.zeros<half_t>(pw), *wl = t.zeros<half_t>(pw);
    half_t *w16h = t.zeros<half_t>((size_t)N * K * 2), *w16l = t.zeros<half_t>((size_t)N * K * 2);
    half_t* xh = t.zeros<half_t>(px);
    unsigned char* xl8 = t.zeros<unsigned char>(px);
    if (t.rc) return t.rc;
    hipLaunchKernelGGL(split_planes_blocked_kernel, dim3(512), dim3(256), 0, h->stream, dA, ah, al, M, K, h->range_flag, 1.0f);
    hipLaunchKernelGGL(split_planes_blocked_kernel, dim3(512), dim3(256), 0, h->stream, dW, wh, wl, N, K, h->range_flag, kWScale);
    hipLaunchKernelGGL(split_planes_k16_kernel, dim3(256), dim3(256), 0, h->stream, dW, w16h, w16l, N, K);
    hipLaunchKernelGGL(split_planes_lo8_kernel, dim3(512), dim3(256), 0, h->stream, dX, xh, xl8, M);
    unsigned char* w8 = dbg_w8(t, dW, N, K);
    if (!w8) return t.rc;
    int rc = 0;
    if (fused == 1) {
        GemmLn2Args g2{ah, w16h, w8, dB, dG, dT, xh, xl8, M, K, 1e-5f, h->range_flag, 0};
        hipError_t e = launch_gemm_ln2_mx(g2, plan_ln_rows(true, M, h->tune), h->stream);
        if (e != hipSuccess) rc = fail(h, JMID_EHIP, hipGetErrorString(e));
    } else {
        GemmHArgs g{};
        g.Ahi = ah; g.Alo = al; g.Whi = wh; g.Wlo = wl; g.W8 = w8; g.bias = dB; g.C = dY; g.ldc = N; g.M = M; g.N = N; g.K = K; g.x2 = mode.x2;
        if (fused == 3) {        // the small-launch kernel with the statistics exchange (gemm_small.hpp, OUT_LNX)
            unsigned long long* xs = t.zeros<unsigned long long>(kLnxWords * sizeof(unsigned));
            const GemmPlan lnx = plan_gemm(GM_MX, EPI_BIAS, OUT_LNX, M, N, K, CallFacts{}, h->tune);      // (an idle handle: nothing else in flight, one launch)
            if (!xs || lnx.shape == GS_NONE) return fail(h, JMID_EINVAL, "jmid_dbg_gemm_ln_mx: shape does not take the small kernel with the statistics exchange");
            g.ln_gamma = dG; g.ln_beta = dT; g.ln_xh = xh; g.ln_xl = nullptr; g.ln_xl8 = xl8; g.ln_xchg = xs; g.ln_eps = 1e-5f; g.ln_no_lo = 0;
            (void)hipMemsetAsync(h->range_flag, 0, sizeof(int), h->stream);
            rc = run_gemm_lnx_small(h, h->stream, KC_GEMM_OUT, g, lnx);
            if (!rc) {
                int flag = 0;
                (void)hipMemcpyAsync(&flag, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream);
                (void)hipStreamSynchronize(h->stream);
                if (flag & 2) rc = fail(h, JMID_EHIP, "jmid_dbg_gemm_ln_mx: a workgroup gave up waiting for its row tile's statistics");
            }
        } else {
            rc = run_gemm_h<EPI_BIAS, OUT_F32>(h, h->stream, KC_GEMM_OUT, g, plan_gemm(GM_MX, EPI_BIAS, OUT_F32, M, N, K, CallFacts{}, h->tune));
            if (!rc) rc = run_add_ln(h, h->stream, nullptr, dY, dG, dT, M, N, xh, reinterpret_cast<half_t*>(xl8), true, 0);
        }
    }
    if (rc) return rc;
    hipLaunchKernelGGL(merge_planes_lo8_kernel, dim3(512), dim3(256), 0, h->stream, xh, xl8, dX, M, (float*)nullptr);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(X, dX, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int jmid_dbg_add_layernorm(jmid_handle_t h, int M, int d, float* X, const float* Y, const float* gamma,
                           const float* beta) {
    if (!h || !X || !Y || !gamma || !beta) return JMID_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    DbgTemps t{h, "jmid_dbg_add_layernorm"};
    float* dX = t.take<float>((size_t)M * d * 4, X);
    float* dY = t.take<float>((size_t)M * d * 4, Y);
    float* dG = t.take<float>((size_t)d * 4, gamma);
    float* dB = t.take<float>((size_t)d * 4, beta);
    if (t.rc) return t.rc;
    if (int rc = run_add_ln(h, h->stream, dX, dY, dG, dB, M, d)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(X, dX, (size_t)M * d * 4, hipMemcpyDeviceToHost));
    return 0;
}

int jmid_dbg_qkv0(jmid_handle_t h, int E, int A, int K, int T, const float* x, const float* hyp, int hyp_width, int step, int precision,
                  float* qkv, float* thyp_row) {
    return h ? dbg_step(h, false, E, A, K, T, x, hyp, hyp_width, step, precision, qkv, thyp_row) : JMID_EINVAL;
}

int jmid_dbg_tail(jmid_handle_t h, int E, int A, int K, int T, const float* X, const float* hyp, int hyp_width, int step, int precision,
                  float* e, float* thyp_row) {
    return h ? dbg_step(h, true, E, A, K, T, X, hyp, hyp_width, step, precision, e, thyp_row) : JMID_EINVAL;
}

int jmid_dbg_seam(jmid_handle_t h, int E, int A, int K, int T, const float* X, const float* x, const float* z, const float* ctx, const float* hyp,
                  int hyp_width, int step, int next_step, int precision, int embed_only, float* x_next, float* hi, float* lo, float* hyp_out,
                  float* thyp_rows, float* coef, int* plan) {
    return h ? dbg_seam(h, E, A, K, T, X, x, z, ctx, hyp, hyp_width, step, next_step, precision, embed_only, x_next, hi, lo, hyp_out, thyp_rows,
                        coef, plan)
             : JMID_EINVAL;
}

int jmid_dbg_layer(jmid_handle_t h, int E, int A, int K, int T, int layer, int precision, const float* X, const int32_t* n_agents, int last,
                   float* hi, float* lo, int* plan) {
    return h ? dbg_layer(h, E, A, K, T, layer, precision, X, n_agents, last, hi, lo, plan) : JMID_EINVAL;
}

int jmid_dbg_noise_words(jmid_handle_t h, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, uint32_t* out, int mem) {
    return noise_entry(h, "jmid_dbg_noise_words", seed, E, rows, T, episode_ids, draw, nullptr, out, mem);
}

}  // extern "C"
#endif  // JMID_DIAGNOSTICS


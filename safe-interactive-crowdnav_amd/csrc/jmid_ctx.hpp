// libjmid_hip.so -- what every translation unit of the host side shares: the handle, error / profiling helpers and the
// internal entry points between the units.  gfx950 only.  No CPU fallback: every entry point that computes needs a HIP device.
// The handle holds what outlives a call; the mode (CallMode), arguments (DenoiseCall, ChainCall, SceneBuild) and lanes of the RUNNING call
// are values passed down, and every block is laid out once by a Carver function that returns typed arrays (call_io, kde_workspace, chain_io,
// grid_block, scene_arrays).
//   jmid_abi.hip      the C ABI proper (include/jmid_hip.h): handle lifetime, encode / denoise / topk / statistics, knobs, stream; the chained
//                     predictor (chain_io, the phases of predict_chain) and the scene build (scene_arrays, build_scene_resident)
//   jmid_weights.hip  weight registry, operand planes (fp16 hi / lo, bf8 images, k16 panels), sampler step tables
//   jmid_planner.hip  chunk plan, step workspace, one net evaluation (net_step), the call plan and the phases of a denoise call (run_network)
//   jmid_profile.hip  per-kernel-class HIP-event profiling
//   jmid_diag.hip     jmid_dbg_* single-kernel, plan and layout entry points (-DJMID_DIAGNOSTICS only)
//   host_mem.hpp      align_up / Carver / Arr, the owning Block (device or pinned) every workspace of the handle is, HostArray, Staging
// Whatever the handle owns is released by ~jmid_ctx: jmid_destroy and a jmid_create that fails half way both end in `delete h`.
#pragma once
#include "../../include/jmid_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "attn_f16x3.hpp"
#include "attn_f32.hpp"
#include "common.hpp"
#include "elementwise.hpp"
#include "encoder.hpp"
#include "eval_stats.hpp"
#include "gemm_f16x3.hpp"
#include "gemm_ln_f16x3.hpp"
#include "gemm_ln2_mx.hpp"
#include "gemm_small.hpp"
#include "gemm_f32.hpp"
#include "kde.hpp"
#include "launch_plan.hpp"
#include "loss.hpp"
#include "noise.hpp"
#include "padded.hpp"
#include "qkv0.hpp"
#include "reject.hpp"
#include "tail_fold.hpp"
#include "scene.hpp"
#include "frames.hpp"
#include "guide.hpp"

using namespace jmid;

enum KClass {
    KC_GEMM_QKV = 0,
    KC_GEMM_OUT,
    KC_GEMM_FF1,
    KC_GEMM_FF2,
    KC_GEMM_TAIL,
    KC_ATTN,
    KC_ADD_LN,
    KC_EMBED,
    KC_OUT_DDIM,
    KC_HYPER,
    KC_ENCODER,
    KC_INTEGRATE,
    KC_METRICS,
    KC_VTRANS,
    KC_LOSS_PREPARE,
    KC_LOSS_REDUCE,
    KC_GUIDE,
    KC_TOPK,
    KC_EVAL_STATS,
    KC_COUNT
};
extern const char* const kClassNames[KC_COUNT];

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
};

struct EvPair {
    hipEvent_t a, b;
};

struct HalfPair {
    half_t* hi = nullptr;
    half_t* lo = nullptr;
};

// The weights one net evaluation reads, resolved to plain pointers once (by jmid_finalize_weights, as it makes the operand planes;
// emptied wherever the buffers they point into go away).  The name-keyed maps of the handle stay the owners of the memory.
struct LinearW {
    const float *W = nullptr, *bias = nullptr;   // fp32 [N, K] and [N]
    HalfPair split;                              // blocked hi / lo fp16 planes (the split-fp16 GEMMs)
    HalfPair k16;                                // k16 panels: out_proj / linear2 at d_model 512 (the row-tile GEMM + LayerNorm), null elsewhere
    const unsigned char* w8 = nullptr;           // bf8 image of W_lo (JMID_PREC_F16MX), null where the shape has none
};
struct NormW {
    const float *gamma = nullptr, *beta = nullptr;
};
struct LayerW {
    LinearW in_proj, out_proj, linear1, linear2;
    NormW norm1, norm2;
};
struct WeightTable {
    std::vector<LayerW> layers;
    LinearW concat1, concat3, concat4, linear;   // (concat1 and linear: fp32 only)
    const float* edge_v = nullptr;               // PEDESTRIAN/edge_influence_encoder.v.weight (the encoder kernel)
};

struct jmid_ctx;
namespace jmid_host {

std::string& thread_error();      // the last error of this thread (jmid_last_error(NULL))
int fail(jmid_ctx* h, int code, const std::string& msg);

#define HIPCHK(h, expr)                                                                               \
    do {                                                                                              \
        hipError_t e__ = (expr);                                                                      \
        if (e__ != hipSuccess)                                                                        \
            return fail(h, JMID_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));            \
    } while (0)

int ensure_arena(jmid_ctx* h, size_t bytes, const char* who);      // jmid_planner.hip
int order_in(jmid_ctx* h, int mem);
int order_out(jmid_ctx* h, int mem);

}  // namespace jmid_host
#include "host_mem.hpp"

namespace jmid_host {
// where the grid of a scene lies in a workspace: the same block in the scene workspace and in the one frames_kernel writes, so that
// one copy moves it (grid_block lays it out)
struct GridBlock {
    Arr<double> human_xy, robot_xy, pose_now;      // [E, F, N, 2] | [E, F, 2] | [E, N, 2]
    size_t xy_bytes = 0;                           // human_xy | robot_xy: what a build from host arrays stages, one copy
};
// The scene workspace (scene_arrays lays it out): the grid block | the padded [E, N, ...] rows jmid_scene_get copies out and
// jmid_predict_scene gathers from | the download block of a build: n_in, in_cluster, robot_in, cv | first_index
struct SceneArrays {
    GridBlock grid;
    Arr<float> x, x_st, nbr_sum, edge_mask, p0;    // [E, N, F, 6] twice | [E, N, 2, F, 6] | [E, N, 2] twice
    Arr<int> n_in;                                 // [E]
    Arr<unsigned char> in_cluster, robot_in;       // [E, N] | [E]
    Arr<double> cv;                                // [E, N, horizon, 2], or none
    size_t down_bytes = 0;                         // n_in ... cv: one copy
    Arr<int> first_index;                          // [E, N], or none
};
}  // namespace jmid_host

struct jmid_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    static constexpr int kMaxLanes = 4;
    hipStream_t lane_stream[kMaxLanes - 1] = {nullptr, nullptr, nullptr};   // extra lanes of the chunk loop
    hipEvent_t ev_fork = nullptr, ev_join[kMaxLanes - 1] = {nullptr, nullptr, nullptr};
    // chunks in flight at once, 1..4 (jmid_set_tuning "lanes").  Two by default: the partially filled last round of one
    // chunk's kernels and its bandwidth-bound kernels overlap with the other chunk's MFMA kernels (+2-4 % traj/s), and the
    // results are bit-identical to one chunk in flight.  (They were not in round 1: a row-wise kernel sharing a CU with
    // attention workgroups of the other lane computed a few wrong values per run - packed-fp32 instructions with crossed
    // operand selects, which the library is no longer built with; build.py, docs/NOTEBOOK.md section 3.)
    int lanes = 2;
    Tuning tune;         // jmid_set_tuning knobs of THIS handle (read as h->tune; `cus` is set by jmid_create)
    hipStream_t caller_stream = nullptr;   // stream device-mode buffers are ordered on (jmid_set_caller_stream)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // captured denoise loops of small calls (one chunk): key = (E, A, K, T, precision) -> executable graph
    struct LoopGraph {
        hipGraphExec_t exec = nullptr;
        char* arena = nullptr;      // the workspace the graph's kernels point into
        bool warm = false;          // the loop ran eagerly once with this key (per-device kernel attributes are set)
    };
    std::map<std::string, LoopGraph> graphs;
    int64_t graph_replays = 0;
    // the positions of the most recent jmid_denoise (integrated into the workspace whether or not they were copied out): what
    // jmid_topk ranks and jmid_eval_statistics scores when they are given no pos pointer
    const float* last_pos = nullptr;
    int last_pos_dims[4] = {0, 0, 0, 0};     // E, A, K, T
    // the velocities that go with last_pos where a block holds them (the accepted block of the rejection entries, when they were asked
    // for), valid only while last_pos == last_vel_pos: jmid_repair_collisions(pos = NULL) rewrites the rows of the samples it repairs
    float* last_vel = nullptr;
    const float* last_vel_pos = nullptr;
    // jmid_denoise_reject_seeded: the accepted set and the loop's tables, in a workspace of its own (it survives the reruns, which reuse the
    // arena; last_pos points into it after the call), and the pinned words of the loop's one download per round
    jmid_host::Block reject_ws;
    jmid_host::Block reject_pin{jmid_host::MEM_PINNED};
    jmid_host::Block kde_ws;                 // jmid_topk's and the statistics entries' own workspace (it must not move the arena last_pos points into)
    // jmid_predict: pinned host staging + device I/O buffers of the chained call, grown on demand
    jmid_host::Block pin{jmid_host::MEM_PINNED};
    jmid_host::Block io_dev;
    // jmid_build_scene: the scene batch it left on the device (padded [E, N, ...] rows; jmid_scene_get copies them out, jmid_predict_scene
    // gathers the in-cluster rows), in a workspace of its own - no other entry point touches it
    struct SceneWs {
        jmid_host::Block dev;
        int E = 0, N = 0;            // E = 0: no scene is resident
        jmid_host::SceneArrays arr;  // the resident arrays, typed pointers into dev (scene_arrays laid them out)
        std::vector<int> n_in;       // [E] in-cluster pedestrians per episode (host copy of arr.n_in, the device counts of the padded chains)
        // stamped: pose_now has the grid block's slot of its own (frames_kernel wrote it); otherwise it is the last frame of the grid
        bool stamped = false;
        int horizon = 0;             // of the resident cv; 0: built without cv
        // jmid_build_scene_var leaves arr.first_index; the other builds leave none and the chained entries then run the encoder without one
        bool has_first() const { return arr.first_index.n != 0; }
    } scene;
    // jmid_build_scene_stamped / _stamped_var: the raw frames and what frames_kernel / track_frames_kernel made of them (grid, pose_now,
    // n_grid, first_frame), in a workspace of its own: a refused build (JMID_EHISTORY, an absent-now track) must not touch the resident scene
    jmid_host::Block frames_dev;
    // the seeded entry points: the call's episode ids on the device (the fill kernel reads them there); the padded ones: its agent counts
    jmid_host::HostArray noise_ids, nag;
    // jmid_wall_statistics / jmid_denoise_reject_walls_seeded: the call's wall segments [L, 4] fp64 on the device (two words per value)
    jmid_host::HostArray wall_seg;
    // jmid_loss: the per-row timesteps of the call on the device (uploaded once per call, as the counts)
    jmid_host::HostArray loss_t;
    // jmid_encode_var: the rows' first history frames; jmid_build_scene_var: the nodes' first frames
    jmid_host::HostArray first_idx;
    int64_t erange_calls = 0;   // calls on this handle that ended with JMID_ERANGE (jmid_erange_count)
    unsigned lnx_epoch = 0;     // launch tag of the small-launch GEMM + LayerNorm with the statistics exchange (gemm_small.hpp, OUT_LNX)
    bool lnx_off = false;       // a workgroup of that kernel once gave up waiting for a partner (range flag bit 1): the handle stays on GEMM + add_ln2
    int64_t lnx_timeouts = 0;   // calls on this handle that ended with JMID_ETIMEOUT for that reason (jmid_timeout_count)
    int net_kind = 1, ctx_dim = 256, tf_layer = 3, nhead = 4, hist_len = 6;
    int d = 512, ff = 1024, dmid = 256, dlow = 128, H = 128;
    HyperLayout hl;
    std::map<std::string, std::vector<size_t>> expected;  // name -> shape
    std::map<std::string, DevBuf> w;
    std::map<std::string, HalfPair> wsplit;  // hi/lo fp16 planes of the GEMM weights (F16X3 path)
    struct W8Image { unsigned char* p = nullptr; };
    std::map<std::string, W8Image> w8;       // JMID_PREC_F16MX: fp8 images of W_lo (w8_image_kernel), keyed like wsplit
    std::map<std::string, HalfPair> w16;     // k16-panel copies of out_proj / linear2 for the fused GEMM + LayerNorm
    WeightTable wt;                          // what the launches read: pointers into the five maps above, valid while `finalized`
    int* range_flag = nullptr;               // device word: an fp16 operand left the fp16 range
    bool weights_in_half_range = true;
    bool finalized = false;
    // derived device buffers
    float* pe = nullptr;
    float* ppe = nullptr;   // [kPeMaxLen, 3 d] image of the positional table under layer 0's in_proj, bias included (qkv0.hpp)
    float* Whyp = nullptr;
    float* bhyp = nullptr;
    float* thyp = nullptr;  // [n_steps, hl.total]
    std::vector<float> time_w;  // host [hl.total][3] time columns of the hyper nets
    // jmid_set_loss_schedule: the forward process per TIMESTEP (index 0 is the reference's padding entry), independent of the sampler's
    // step table - host copies, and on the device the time table [n_t, hl.total] (the expression of thyp), c0 | c1 [2 n_t] and the
    // zeroed row of hl.total floats a loss call hands the kernels as their thyp
    std::vector<float> loss_beta, loss_c0, loss_c1;
    float* loss_tt = nullptr;
    float* loss_c = nullptr;
    float* zero_thyp = nullptr;
    float* lstmT[3][3] = {{nullptr}};  // [hist, edge_ped, edge_robot] x [WihT, WhhT, b]
    float* attW1T = nullptr;
    float* attW2T = nullptr;
    // sampler step table (host): DDIM coefficients, or DDPM ones when ddpm is set
    std::vector<float> beta, c_e, c_x, n_x, n_e;
    bool ddpm = false;
    std::vector<float> p_c0, p_c1, p_sigma;
    std::vector<int> p_noise;
    jmid_host::Block arena;     // the workspace of the denoise call (grown by ensure_arena only)
    // I/O staging
    int chunk_eps = 0;
    // profiling
    uint32_t prof_mask = 0;
    std::vector<EvPair> prof_ev[KC_COUNT];
    std::vector<EvPair> ev_pool;
    double prof_ms[KC_COUNT] = {0};
    int64_t prof_n[KC_COUNT] = {0};
    std::string err;
    jmid_ctx() = default;
    jmid_ctx(const jmid_ctx&) = delete;
    ~jmid_ctx();                // everything above that was created; nothing for a handle that never created anything (jmid_abi.hip)
};

constexpr size_t kLnxWords = 2 * jmid::SM_LNX_GRANULES;      // 32-bit words of the exchange granules (8 bytes each) of the small-launch GEMM + LayerNorm per step workspace (gemm_small.hpp, OUT_LNX)

namespace jmid_host {

inline hipStream_t stream_of(jmid_ctx* h) { return h->stream; }
inline int reserve_block(jmid_ctx* h, Block& b, size_t need, const char* who) {
    return &b == &h->arena ? ensure_arena(h, need, who) : b.reserve(h, need, who);
}

// The arithmetic mode of one call, made from its `precision` argument by call_mode - the one place that says which precisions exist -
// and passed down by value: the step plan holds it, the rules that run before a step plan take it as a parameter.
struct CallMode {
    int precision = JMID_PREC_F32;
    bool split = false;     // a split-fp16 mode: the residual stream lives in hi / lo planes
    int x2 = 0;             // F16X2 or F16MX: two MFMA terms (everything of F16MX that is not on the fp8 path runs as F16X2)
    int mx = 0;             // F16MX
    // what the GEMMs are planned for (plan_gemm keeps F16MX exactly where a weight has its bf8 image: N a multiple of 128, K of 64 -
    // jmid_weights.hip makes one from N % 32 == 0 and K % 64 == 0)
    GemmMode gemm = GM_X3;
};
inline bool call_mode(int precision, CallMode* m) {
    if (precision != JMID_PREC_F32 && precision != JMID_PREC_F16X3 && precision != JMID_PREC_F16X2 && precision != JMID_PREC_F16MX) return false;
    const int mx = precision == JMID_PREC_F16MX, x2 = precision == JMID_PREC_F16X2 || mx;
    *m = CallMode{precision, precision != JMID_PREC_F32, x2, mx, !x2 ? GM_X3 : mx ? GM_MX : GM_X2};
    return true;
}

struct ProfScope {
    jmid_ctx* h;
    int cls;
    hipStream_t stream;
    bool on;
    EvPair ev;
    ProfScope(jmid_ctx* h_, int cls_, hipStream_t s) : h(h_), cls(cls_), stream(s), on((h_->prof_mask >> cls_) & 1u) {
        if (on) {
            if (!h->ev_pool.empty()) {
                ev = h->ev_pool.back();
                h->ev_pool.pop_back();
            } else {
                hipEventCreate(&ev.a);
                hipEventCreate(&ev.b);
            }
            hipEventRecord(ev.a, stream);
        }
    }
    ~ProfScope() {
        if (on) {
            hipEventRecord(ev.b, stream);
            h->prof_ev[cls].push_back(ev);
        }
    }
};

inline size_t numel(const std::vector<size_t>& s) {
    size_t n = 1;
    for (size_t v : s) n *= v;
    return n;
}

// jmid_weights.hip
void register_shapes(jmid_ctx* h);
int dev_alloc_copy(jmid_ctx* h, float** out, const std::vector<float>& host);
int fetch_host(jmid_ctx* h, const std::string& name, std::vector<float>& out);
std::vector<float> time_table(const jmid_ctx* h, const std::vector<float>& beta);      // [beta.size(), hl.total]: thyp's and the loss schedule's
int upload_time_table(jmid_ctx* h);
int upload_loss_schedule(jmid_ctx* h);
int make_w8(jmid_ctx* h, const float* dW, int N, int K, jmid_ctx::W8Image* out);
int w8_image(jmid_ctx* h, const float* dW, int N, int K, unsigned char* out);      // ... into a buffer of the caller's (N K bytes)
void free_planes(jmid_ctx* h);
void free_derived(jmid_ctx* h);     // the buffers jmid_finalize_weights derives from the weights
void free_weights(jmid_ctx* h);     // the planes, the derived buffers, the weights themselves, the step table and the range flag
// jmid_planner.hip
void drop_graphs(jmid_ctx* h);
void sync_lanes(jmid_ctx* h);
std::vector<int> plan_chunks(const jmid_ctx* h, const CallMode& m, int E, int tokens_per_episode);
int check_ready(jmid_ctx* h);
// seeded noise of a call (noise.hpp): x_T is draw 0 and the z of step-table entry i draw i + 1, filled on the device; `ids` [E] is a HOST array
struct SeedArgs {
    uint64_t seed;
    const uint32_t* ids;
    int draw = 0;                         // the draw number x_T is (jmid_denoise_reject_seeded: draw0 + the round); DDIM only when not 0
};
int fill_noise(jmid_ctx* h, uint64_t seed, const unsigned* ids_dev, int E, size_t n, int draw, float* out, unsigned* words, hipStream_t stream);
// ... of a padded batch: the real rows of out [E, K * A, T, 2], every episode's own compact draw; the padded rows are left alone
int fill_noise_padded(jmid_ctx* h, uint64_t seed, const unsigned* ids_dev, const int* n_agents_dev, int E, int A, int K, int T, int draw, float* out,
                      hipStream_t stream);
// What a loss call (jmid_loss / jmid_loss_seeded; loss.hpp) adds to a single-step call with K = 1: x_in is x0
struct LossCall {
    const int32_t* t = nullptr;           // HOST [E, A] timesteps, 1 .. n_t - 1
    const float* e = nullptr;             // [E, A, T, 2], or null: draw 0 of the counter generator with rows = A
    const SeedArgs* seeded = nullptr;
    double *loss_out = nullptr, *row_out = nullptr;      // [2]; [E, A] or null
};
// What a guided call (jmid_denoise_guided*; guide.hpp) adds to a denoise call: the rule's arguments and the per-entry weights.  A value
// of the call like everything else here: nothing of it stays on the handle
struct GuideCall {
    double threshold = 0.0, margin = 0.0, tau = 0.0;
    const double* weights = nullptr;      // HOST [n_steps], metres; 0: no launch behind that entry
    int n_inner = 0;
    int L = 0;
    const double* walls = nullptr;        // [L, 4] on the DEVICE (upload_walls), null at L = 0
    double wall_radius = 0.0;
    float* guide_out = nullptr;           // [E, K, 2] where `mem` says, or null
};
// One denoise call (or, with single_step >= 0, one net evaluation -> e_out) as its entry point states it
struct DenoiseCall {
    int E, A, K, T, precision, mem;
    const float *x_in = nullptr, *ctx = nullptr, *p0 = nullptr;     // x_in null: seeded
    float dt = 0.f;
    float *vel_out = nullptr, *pos_out = nullptr, *e_out = nullptr;
    int single_step = -1;
    const float* z = nullptr;             // DDPM noise [n_steps, M, 2] of the caller
    const SeedArgs* seeded = nullptr;     // ... or x_T and the DDPM z drawn on the device
    bool chained = false;                 // a stage of jmid_predict: no caller-stream ordering, no flag round trip
    // a padded call (padded.hpp): HOST array [E], 1 <= n_agents[e] <= A - episode e has n_agents[e] real agents, the rows of the others
    // are zeroed on entry and NaN in every output; JMID attention takes the key-mask words.  DDIM only.
    const int32_t* n_agents = nullptr;
    // ... whose counts already lie on the device (the padded scene chains: the n_in the build kernel wrote): n_agents is the host copy
    // the checks read, and nothing is uploaded.  With `seeded`, x_T is the padded fill of noise.hpp (DDIM only).
    const int* n_agents_dev = nullptr;
    const LossCall* loss = nullptr;       // a loss call: per-row timesteps folded into hyp, a zero row as thyp, e_out may be null
    // a guided call: every step embeds at its head (no fused seam), the guide kernel follows each entry whose weight is > 0 on the chunk's
    // stream, never captured.  DDIM only, p0 required
    const GuideCall* guide = nullptr;
    const char* who = "jmid_denoise";     // the entry point that was called (error texts)
};
// What a constrained chain (jmid_predict_constrained, jmid_predict_scene_constrained, jmid_forecast_scene_constrained) carries through its
// phases: the guidance of the denoise stage, the repair between the denoise stage and the ranking, the walls both may read, and the HOST
// report arrays that come back with the one download.  A value of the call: nothing of it stays on the handle
struct ChainConstraints {
    double threshold = 0.0;
    const double* guide_weights = nullptr;      // HOST [n_steps] or null: no guidance
    int n_inner = 0;
    double guide_margin = 0.0, guide_tau = 0.0;
    bool guide_walls = false;                   // the guidance takes the wall terms (L > 0)
    bool repair = false;
    double margin = 0.0, tau = 0.0, step = 0.0;
    int max_iter = 0;
    bool repair_walls = false;                  // the repair is jmid_repair_collisions_walls' (L > 0)
    int L = 0;
    const double* walls = nullptr;              // HOST [L, 4]: sent once per call, for both mechanisms
    double wall_radius = 0.0;
    float *guide_out = nullptr, *sample_out = nullptr, *wall_out = nullptr;      // HOST [E, K, 2] | [E, K, 4] | [E, K, 2], each may be null
    int32_t* episode_out = nullptr;                                             // HOST [E, 3] or null
    bool guided() const { return guide_weights != nullptr; }
    bool walled() const { return L > 0 && ((guided() && guide_walls) || (repair && repair_walls)); }
};
// One chained call (jmid_predict*, jmid_predict_scene*, jmid_forecast_scene*) as its entry point states it: upload, encoder -> denoise
// loop -> integrator -> top-k (-> assembly) on the stream, one download.  The modes are members, not null pointers read at a distance.
struct ChainCall {
    int E, A, K, T, k, precision;
    float dt = 0.f;
    const char* who = "jmid_predict";     // the entry point that was called (error texts)
    bool scene = false;                   // the in-cluster rows of the resident scene are gathered on the device: no host inputs but the noise and bw
    bool forecast = false;                // scene only: assemble_kernel follows, forecasts_out / logw_out are the download and sel / logw / pos stay on the device
    bool padded = false;                  // mixed agent counts, A the largest: n_agents says them
    const float *x_st = nullptr, *nbr_sum = nullptr, *edge_mask = nullptr, *p0 = nullptr;      // HOST inputs (scene: none)
    const float* x_T = nullptr;           // the noise: HOST [E, K A, T, 2], or
    const SeedArgs* seeded = nullptr;     // ... (scene only) draw 0 of noise.hpp, filled into x_T's slot on the device
    const float* bw = nullptr;            // HOST [T] or null; read when k < K
    float *sel = nullptr, *logw = nullptr, *pos_out = nullptr;      // k < K: sel, logw; pos_out optional then
    double *forecasts_out = nullptr, *logw_out = nullptr;           // forecast: [E, N, k, T+1, 2] and [E, N, k]
    // padded: HOST [E].  Host arrays: the caller's counts, uploaded by the denoise stage - the padded agents' rows go through the
    // encoder as the caller left them (its rows are independent) and the denoise stage zeroes their ctx, x_T and p0.  Scene: the host
    // copy of the resident scene's counts; the stages read the device counts the build kernel wrote (nothing is uploaded for them),
    // the gather zeroes the padded rows and a seeded x_T is the padded fill
    const int32_t* n_agents = nullptr;
    const ChainConstraints* cons = nullptr;      // the constrained entries only: null for every other chain
    bool rank() const { return k < K; }
};
// The I/O block of a chained call as chain_io lays it out, in device memory or (ctx and first_index absent, and after the assembled
// arrays of a forecast nothing) in the pinned block
struct ChainIo {
    Arr<float> x_st, nbr_sum, edge_mask, x_T, p0, bw;      // the upload block: [E A, Th, 6] | [E A, 2, Th, 6] | [E A, 2] | [E, K A, T, 2] | [E, A, 2] | [T] or none
    size_t up_bytes = 0;
    Arr<float> ctx;                                        // [E A, 2 H]
    Arr<int> flag;                                         // the download block: the range flag's word |
    Arr<double> forecasts, logw_d;                         // forecast: [E, N, k, T+1, 2] | [E, N, k] |
    Arr<float> guide, rsample;                             // constrained: the reports [E, K, 2] | [E, K, 4] |
    Arr<int> repisode;                                     //   [E, 3] |
    Arr<float> rwall;                                      //   [E, K, 2] |
    Arr<float> sel, logw, pos;                             // k < K: [E, A, k, T, 2] | [E, A, k] | pos_out given: [E, K, A, T, 2]
    size_t down_bytes = 0;                                 // flag ... pos; forecast: flag ... logw_d (constrained: ... rwall)
    Arr<int> first_index;                                  // a scene with one: [E A]
    Arr<double> gate;                                      // a chain with repair: the predicates' lean per-sample values [E, K, 2] (with walls: twice)
    size_t up_bytes_from(const Arr<float>& a) const { return up_bytes - (size_t)((const char*)a.p - (const char*)x_st.p); }      // the rest of the upload block from `a` on
};
// One scene build (jmid_build_scene*, and the second half of jmid_build_scene_stamped*) as its entry point states it
enum SceneSource {
    SCENE_HOST_ARRAYS,       // human_xy [E, F, N, 2], robot_xy [E, F, 2]: host arrays, staged
    SCENE_DEVICE_ARRAYS,     // ... device arrays
    SCENE_DEVICE_GRID,       // human_xy is a device GridBlock (grid + pose_now, as frames_kernel left it), robot_xy unused
};
struct SceneBuild {
    const char* who;
    int E, N, F;
    SceneSource src;
    const double *human_xy, *robot_xy;
    const int32_t* first_frame = nullptr;      // a HOST array [E, N + 1], checked by the entry, or null: uploaded ahead of the kernel, which then leaves first_index
    bool allow_absent = false;                 // first_frame may hold -1 for a pedestrian (not in the scene; jmid_build_scene_absent, _stamped_coast)
    double time_step = 0.0;
    int horizon = 0, force_all_in_cluster = 0;
    uint8_t *in_cluster_out = nullptr, *robot_in_cluster_out = nullptr;
    int* n_in_out = nullptr;
    double* cv_out = nullptr;                  // null: no cv (and no jmid_forecast_scene on this scene)
    int mem = JMID_MEM_HOST;                   // where the four outputs live
};
// the counts of a padded call: checked by its entry before anything is enqueued (JMID_EINVAL: null, or a count outside 1..A), then
// uploaded through h->nag on h->stream
int check_n_agents(jmid_ctx* h, const char* who, const int32_t* n_agents, int E, int A);
int run_network(jmid_ctx* h, DenoiseCall a);      // (by value: its host inputs become their uploads)
int dbg_step(jmid_ctx* h, bool tail, int E, int A, int K, int T, const float* in, const float* hyp, int hyp_width, int step, int precision,
             float* out, float* thyp_row);      // jmid_dbg_qkv0 (tail = false) / jmid_dbg_tail: -DJMID_DIAGNOSTICS only
int dbg_layer(jmid_ctx* h, int E, int A, int K, int T, int layer, int precision, const float* X, const int32_t* n_agents, int last,
              float* hi, float* lo, int* plan);      // jmid_dbg_layer: -DJMID_DIAGNOSTICS only
int dbg_seam(jmid_ctx* h, int E, int A, int K, int T, const float* X, const float* x, const float* z, const float* ctx, const float* hyp,
             int hyp_width, int step, int next_step, int precision, int embed_only, float* x_next, float* hi, float* lo, float* hyp_out,
             float* thyp_rows, float* coef, int* plan);      // jmid_dbg_seam: -DJMID_DIAGNOSTICS only
int flagged_call(jmid_ctx* h, int flag);     // the status of a call whose range flag came back set (JMID_ETIMEOUT / JMID_ERANGE)
int launch_episode_metrics(jmid_ctx* h, const float* pos, const float* gt, float* out, int E, int K, int A, int T);
// jmid_abi.hip
size_t chain_io(const jmid_ctx* h, const ChainCall& c, char* base, ChainIo* out, bool pinned);
size_t scene_arrays(int E, int N, int F, int horizon, bool has_first, char* base, SceneArrays* out);
int noise_entry(jmid_ctx* h, const char* who, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, float* out,
                unsigned* words, int mem);
// jmid_profile.hip
int prof_collect(jmid_ctx* h);

}  // namespace jmid_host
using namespace jmid_host;

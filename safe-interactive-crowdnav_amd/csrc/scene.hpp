// Scene batch on the device: track positions on the time_step grid -> the arrays the encoder consumes.
//
// The device twin of scene.py::build_scenes_batched (mid_sim_wrapper.py:313-437, MID/dataset/preprocessing.py:428-620,
// MID/environment/scene_graph.py:111-250, the reductions of MID/models/encoders/mgcvae.py:726-768), in the same operation order:
//   1. last-frame distance matrix, near = d < 3
//   2. cluster means: the members summed in ascending node order, divided by their count
//   3. the pedestrian whose cluster mean is nearest the robot (the first minimum); in_cluster = its row of `near`
//   4. node states [pos, vel, acc] by first differences, first element duplicated, divided by time_step
//   5. scene graph over the last three frames among the in-cluster nodes: type-valued adjacency (pedestrian 1, robot 2, diagonal 0),
//      addition filter (0.25, 0.5, 0.75, 1) with clamp 1, zero where not adjacent now, connected = scaling > 1e-2
//   6. per pedestrian row x, x_st, p0, edge_mask (the same clamped sum for both edge types: scene_graph.py:293-299 does not filter the edge
//      values by type) and per edge type the fp32 sum over the connected neighbours, in node order, of their standardised state
//      relative to the ego's present state (the robot is edge type 1)
//   7. constant-velocity forecasts of every pedestrian by sequential cumulative sum
// fp64 wherever scene.py computes in float64, fp32 exactly where it casts.  Every decision (< 3, <= 3, > 1e-2, the first minimum) compares
// correctly rounded + - * / sqrt results, so the kernel is compiled WITHOUT FMA contraction (a contracted dx * dx + dy * dy moves a
// distance by an ulp, and tests/golden/wrapper_jmid_entering.npz has a pair 4.4e-16 from the radius): the outputs are bit-identical to
// the host twin's whenever the chosen cluster does not hinge on the summation order of step 2.
//
// Short histories (first_frame [E, N + 1], robot first; null: every node has all F frames): node j is present on frames first_frame[j] .. F-1.
//   * its velocity and acceleration are the first differences over ITS span (data_utils.py:24-37; a single frame: both zero); x and x_st
//     are NaN in front of the span (node.get(..., padding=nan)), and a position in front of it is never read
//   * the scene graph sees NaN there (environment/scene.py:84-106): a NaN distance is not <= radius, no adjacency on that frame
//   * a connected neighbour's state is taken with padding 0.0 and THEN standardised relative to the ego (preprocessing.py:531-550): on a
//     frame where it is absent it adds (0 - ego_now) / std in all six columns
//   * a pedestrian with ONE frame is never an ego row (in_cluster 0, no graph row, its constant-velocity row its position repeated) but
//     still counts in the cluster choice and as a neighbour (present_nodes: min_history_timesteps 1 for the egos, 0 for the graph)
// With first_frame null every operation and its order are the ones above.
//
// A node with no frame (first_frame[1 + j] == -1, jmid_build_scene_absent; never the robot): pedestrian j is NOT IN THE SCENE.  His
// positions are never read (`here` is false on every frame), he is no candidate of step 3 (his rdist would be 0 / 0, and a NaN is
// the minimum), no member of a cluster mean (a NaN distance is not < 3), not in `inc` - so no graph node and nobody's neighbour -, no
// ego row, and his output rows are in_cluster 0, first_index -1, NaN in every float.  Every other lane does what it does when his
// column is removed: the members are summed in ascending node order and a non-member adds nothing (a neighbour outside `conn` adds
// +-0 to a sum that started at +0: the bits stay).  A first_frame without -1 takes none of these branches.
//
// One workgroup of one wavefront per episode, one lane per node (node 0 the robot, 1 .. N the pedestrians: N + 1 <= 64); the node states
// are staged in LDS.  The kernel is latency-bound and tiny.  A second kernel gathers the in-cluster rows, in ascending track id, into the
// dense [E * A, ...] layout the encoder and the integrator read (jmid_predict_scene).
#pragma once
#include "common.hpp"

namespace jmid {

constexpr int SCN_LANES = 64;         // one wavefront: one lane per node
constexpr int SCN_MAX_F = 16;         // history frames (== ENC_MAX_TH)
constexpr int SCN_MAX_H = 24;         // horizon of the constant-velocity forecasts

struct SceneArgs {
    const double* human_xy;       // [E, F, N, 2]
    const double* robot_xy;       // [E, F, 2]
    const int* first_frame;       // [E, N + 1] first present frame of every node (robot first), 0 .. F-1; null: 0.  -1 (a pedestrian, the
                                  // host has checked: not all of an episode's): not in the scene
    int* first_index;             // [E, N] the pedestrians' first_frame, as the encoder reads it (written only with first_frame)
    float* x;                     // [E, N, F, 6]
    float* x_st;                  // [E, N, F, 6]
    float* nbr_sum;               // [E, N, 2, F, 6]
    float* edge_mask;             // [E, N, 2]
    float* p0;                    // [E, N, 2]
    unsigned char* in_cluster;    // [E, N]
    unsigned char* robot_in;      // [E]
    int* n_in;                    // [E]
    double* cv;                   // [E, N, horizon, 2] or null
    double dt;
    int E, N, F, horizon, force_all;
};

inline size_t scene_lds(int F) { return sizeof(double) * (size_t)F * SCN_LANES * 6; }

static __global__ __launch_bounds__(SCN_LANES) void scene_kernel(SceneArgs g) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char scn_lds_raw[];
    __shared__ double rdist[SCN_LANES];
    __shared__ unsigned long long nearm[SCN_LANES];
    __shared__ int sfirst[SCN_LANES];
    double* S = reinterpret_cast<double*>(scn_lds_raw);       // [F, 64, 6] node states
    const int i = threadIdx.x, e = blockIdx.x;
    const int N = g.N, F = g.F, n = N + 1;
    const double dt = g.dt;
    auto st = [&](int t, int node, int c) -> double& { return S[((size_t)t * SCN_LANES + node) * 6 + c]; };
    // positions: robot first, like the track ids (-1, 0, 1, ...)
    const double* hum = g.human_xy + (size_t)e * F * N * 2;
    const double* rob = g.robot_xy + (size_t)e * F * 2;
    const int* ffe = g.first_frame ? g.first_frame + (size_t)e * n : nullptr;
    const double nan64 = __builtin_nan("");
    for (int q = i; q < F * n * 2; q += SCN_LANES) {
        const int c = q & 1, node = (q >> 1) % n, t = (q >> 1) / n;
        const bool here = !ffe || (ffe[node] >= 0 && t >= ffe[node]);
        st(t, node, c) = !here ? nan64 : node == 0 ? rob[t * 2 + c] : hum[((size_t)t * N + (node - 1)) * 2 + c];
    }
    sfirst[i] = ffe && i < n ? ffe[i] : 0;
    __syncthreads();
    // step 4 (every lane its own node, over its own span) and steps 1-2
    if (i < n && sfirst[i] < 0) {
        // no frame: NaN states (the positions are NaN already), near nobody
        for (int t = 0; t < F; ++t)
            for (int c = 2; c < 6; ++c) st(t, i, c) = nan64;
        rdist[i] = nan64;
        nearm[i] = 0;
    } else if (i < n) {
        const int f0 = sfirst[i];
        for (int c = 0; c < 2; ++c) {
            if (f0 < F - 1) {
                for (int t = f0 + 1; t < F; ++t) st(t, i, 2 + c) = (st(t, i, c) - st(t - 1, i, c)) / dt;
                st(f0, i, 2 + c) = st(f0 + 1, i, 2 + c);
                for (int t = f0 + 1; t < F; ++t) st(t, i, 4 + c) = (st(t, i, 2 + c) - st(t - 1, i, 2 + c)) / dt;
                st(f0, i, 4 + c) = st(f0 + 1, i, 4 + c);
            } else {
                st(f0, i, 2 + c) = 0.0;
                st(f0, i, 4 + c) = 0.0;
            }
            for (int t = 0; t < f0; ++t) st(t, i, 2 + c) = st(t, i, 4 + c) = nan64;
        }
        const double px = st(F - 1, i, 0), py = st(F - 1, i, 1);
        unsigned long long m = 0;
        double sx = 0.0, sy = 0.0;
        int cnt = 0;
        for (int j = 0; j < n; ++j) {
            const double qx = st(F - 1, j, 0), qy = st(F - 1, j, 1);
            const double dx = px - qx, dy = py - qy;
            if (sqrt(dx * dx + dy * dy) < 3.0) {
                m |= 1ull << j;
                sx = sx + qx;
                sy = sy + qy;
                ++cnt;
            }
        }
        const double mx = sx / (double)cnt - st(F - 1, 0, 0), my = sy / (double)cnt - st(F - 1, 0, 1);
        rdist[i] = sqrt(mx * mx + my * my);
        nearm[i] = m;
    }
    __syncthreads();
    // step 3: the first minimum over the pedestrians that are in the scene (np.argmin: a NaN counts as the minimum)
    unsigned long long inc = n == 64 ? ~0ull : (1ull << n) - 1;
    if (!g.force_all) {
        int best = -1;
        double bv = 0.0;
        for (int j = 1; j < n; ++j) {
            if (sfirst[j] < 0) continue;
            const double r = rdist[j];
            if (best < 0 || (bv == bv && (r < bv || r != r))) { bv = r; best = j; }
        }
        inc = best < 0 ? 0ull : nearm[best];
    } else {
        for (int j = 1; j < n; ++j)
            if (sfirst[j] < 0) inc &= ~(1ull << j);
    }
    // the ego rows: the in-cluster pedestrians with at least two frames (all of them without first_frame)
    unsigned long long ego = inc & ~1ull;
    for (int j = 1; j < n; ++j)
        if (sfirst[j] > F - 2 || sfirst[j] < 0) ego &= ~(1ull << j);
    if (i == 0) {
        g.robot_in[e] = (unsigned char)(inc & 1ull);
        g.n_in[e] = __popcll(ego);
    }
    if (i < 1 || i >= n) return;
    const size_t row = (size_t)e * N + (i - 1);
    const bool in_me = (ego >> i) & 1ull;
    const int f0 = sfirst[i];
    g.in_cluster[row] = in_me ? 1 : 0;
    if (ffe) g.first_index[row] = f0;
    const float nan32 = __builtin_nanf("");
    if (f0 < 0) {                                             // not in the scene: NaN rows
        for (int q = 0; q < F * 6; ++q) g.x[row * F * 6 + q] = g.x_st[row * F * 6 + q] = nan32;
        for (int q = 0; q < 2 * F * 6; ++q) g.nbr_sum[row * 2 * F * 6 + q] = nan32;
        for (int q = 0; q < 2; ++q) g.edge_mask[row * 2 + q] = g.p0[row * 2 + q] = nan32;
        if (g.cv)
            for (int q = 0; q < g.horizon * 2; ++q) g.cv[row * g.horizon * 2 + q] = nan64;
        return;
    }
    // step 5: this pedestrian's row of the edge scaling, as a mask of connected nodes and the fp32 sum of their values
    unsigned long long conn = 0;
    float ev = 0.0f;
    if (in_me) {
        for (int j = 0; j < n; ++j) {
            if (j == i || !((inc >> j) & 1ull)) continue;
            const double ty = j == 0 ? 2.0 : 1.0;
            double a[3];
            for (int f = 0; f < 3; ++f) {
                const int t = F - 3 + f;
                const double dx = st(t, i, 0) - st(t, j, 0), dy = st(t, i, 1) - st(t, j, 1);
                a[f] = sqrt(dx * dx + dy * dy) <= 3.0 ? ty : 0.0;
            }
            double s = fmin(0.25 * a[2] + 0.5 * a[1] + 0.75 * a[0], 1.0);
            if (a[2] == 0.0) s = 0.0;
            if (s > 1e-2) {
                conn |= 1ull << j;
                ev = ev + (float)s;
            }
        }
    }
    const float em = fminf(ev, 1.0f);
    g.edge_mask[row * 2] = em;
    g.edge_mask[row * 2 + 1] = em;
    // step 6
    const double std6[6] = {3.0, 3.0, 2.0, 2.0, 1.0, 1.0};
    float* xo = g.x + row * F * 6;
    float* xs = g.x_st + row * F * 6;
    float* nb = g.nbr_sum + row * 2 * F * 6;
    double now[6];
    for (int c = 0; c < 6; ++c) now[c] = st(F - 1, i, c);
    g.p0[row * 2] = (float)now[0];
    g.p0[row * 2 + 1] = (float)now[1];
    for (int t = 0; t < F; ++t)
        for (int c = 0; c < 6; ++c) {
            const double v = st(t, i, c);
            xo[t * 6 + c] = t < f0 ? nan32 : (float)v;
            xs[t * 6 + c] = t < f0 ? nan32 : (float)((v - (c < 2 ? now[c] : 0.0)) / std6[c]);
            // every node is added, an unconnected one with weight 0, as the host twin does (the sums start at +0.0)
            float acc_ped = 0.0f, acc_rob = 0.0f;
            for (int j = 0; j < n; ++j) {
                const float rel = (float)(((t < sfirst[j] || sfirst[j] < 0 ? 0.0 : st(t, j, c)) - now[c]) / std6[c]);
                const float w = (conn >> j) & 1ull ? 1.0f : 0.0f;
                if (j == 0) acc_rob = acc_rob + rel * w;
                else acc_ped = acc_ped + rel * w;
            }
            nb[t * 6 + c] = acc_ped;
            nb[(F + t) * 6 + c] = acc_rob;
        }
    // step 7
    if (g.cv) {
        double* o = g.cv + row * g.horizon * 2;
        for (int c = 0; c < 2; ++c) {
            const double step = now[2 + c] * dt;
            double cs = step;
            for (int hh = 0; hh < g.horizon; ++hh) {
                o[hh * 2 + c] = now[c] + cs;
                cs = cs + step;
            }
        }
    }
}

inline hipError_t launch_scene(const SceneArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(scene_kernel, dim3(g.E), dim3(SCN_LANES), scene_lds(g.F), st, g);
    return hipGetLastError();
}

// the in-cluster rows of the padded [E, N, ...] scene arrays, in ascending track id, as dense [E * A, ...] rows
struct SceneGatherArgs {
    const unsigned char* in_cluster;      // [E, N]
    const float *x_st, *nbr_sum, *edge_mask, *p0;     // padded
    float *o_x_st, *o_nbr_sum, *o_edge_mask, *o_p0;   // dense
    const int* first_index;               // [E, N] padded, or null (a scene built without first_frame)
    int* o_first_index;                   // [E * A] dense (written only with first_index)
    int E, N, A, F;
    int pad;                              // the padded chains: an episode with fewer than A rows gets zeros in the rest (0: they are left alone)
};

static __global__ __launch_bounds__(SCN_LANES) void scene_gather_kernel(SceneGatherArgs g) {
    __shared__ int src_row[SCN_LANES];
    const int i = threadIdx.x, e = blockIdx.x;
    const int N = g.N, A = g.A, F = g.F;
    const bool on = i < N && g.in_cluster[(size_t)e * N + i];
    const unsigned long long m = __ballot(on);
    const int rank = __popcll(m & ((1ull << i) - 1));
    if (on && rank < A) src_row[rank] = i;
    __syncthreads();
    const int rows = min(A, (int)__popcll(m));        // (the host has checked that the count is A)
    const int nx = F * 6, nn = 2 * F * 6;
    for (int r = 0; r < rows; ++r) {
        const size_t s = (size_t)e * N + src_row[r], d = (size_t)e * A + r;
        for (int q = i; q < nx; q += SCN_LANES) g.o_x_st[d * nx + q] = g.x_st[s * nx + q];
        for (int q = i; q < nn; q += SCN_LANES) g.o_nbr_sum[d * nn + q] = g.nbr_sum[s * nn + q];
        if (i < 2) {
            g.o_edge_mask[d * 2 + i] = g.edge_mask[s * 2 + i];
            g.o_p0[d * 2 + i] = g.p0[s * 2 + i];
        }
        if (g.first_index && i == 0) g.o_first_index[d] = g.first_index[s];
    }
    // padded rows: zeros, never what the previous call left there - a finite encoder row that starts at frame 0
    for (int r = g.pad ? rows : A; r < A; ++r) {
        const size_t d = (size_t)e * A + r;
        for (int q = i; q < nx; q += SCN_LANES) g.o_x_st[d * nx + q] = 0.0f;
        for (int q = i; q < nn; q += SCN_LANES) g.o_nbr_sum[d * nn + q] = 0.0f;
        if (i < 2) {
            g.o_edge_mask[d * 2 + i] = 0.0f;
            g.o_p0[d * 2 + i] = 0.0f;
        }
        if (g.first_index && i == 0) g.o_first_index[d] = 0;
    }
}

inline hipError_t launch_scene_gather(const SceneGatherArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(scene_gather_kernel, dim3(g.E), dim3(SCN_LANES), 0, st, g);
    return hipGetLastError();
}

}  // namespace jmid

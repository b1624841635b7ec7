// Stamped frames in, predict_ret_best arrays out: the two ends of the predictor call that surround the scene batch (scene.hpp).
//
// frames_kernel: the device twin of scene.py::frame_table_frames (mid_sim_wrapper.py:244-298) for E independent episodes whose R raw
// frames carry one stamp each, shared by every human and the robot (what update_state_hists produces), in the same operation order:
//   1. pose_now = the human positions of the last PUSHED valid frame, before anything is dropped or sorted (agent_df.tail(1))
//   2. a frame with a NaN stamp or a NaN coordinate is dropped (dropna)
//   3. stable sort by stamp (equal stamps keep push order): never materialised - "later in sorted order" is the comparison
//      (stamp, push index) wherever the order matters
//   4. ns = (int64) trunc(stamp * 100), w = round(time_step * 100), bin b = floor((ns_last - ns) / w) counted back from the newest stamp
//   5. only the bins 0 .. F-1 are produced (nb = max(b) + 1 rows are never materialised: one stale frame makes nb huge).  A bin holds the
//      LAST sorted frame that falls into it; an empty bin is interpolated between the nearest filled older bin (which may lie beyond F-1)
//      and the nearest filled newer bin, each by its last frame, in index space x = nb-1-b:
//          slope = (y1 - y0) / (x1 - x0);  y = slope * (x - x0) + y0           fp64, no FMA contraction, this association
//      which is what np.interp computes.  Bin 0 and the bin of the oldest kept frame are always filled.
//   6. n_grid = min(F, nb) grid frames, oldest first in rows 0 .. n_grid-1 of the outputs; the rows behind them are zero
// One workgroup of one wavefront per episode, as scene_kernel; a lane per raw frame (R <= 64) or per bin (F <= 16) where the work is
// per frame or per bin, all lanes striding over (row, column) where it is per value.  LDS holds the per-frame stamps and bins and the
// per-bin sources ([R] and [F] entries: frames_lds); the coordinates themselves (R x (2N + 2) doubles, N <= 63) are read where they lie.
// Latency-bound and tiny: clarity before cleverness.
//
// track_frames_kernel: the frame table PER TRACK (jmid_build_scene_stamped_var; the device twin of scene.py::frame_table_tracks, in its
// operation order).  A NaN coordinate of pedestrian j means "track j was not seen in this frame" and drops nothing:
//   1. pose_now as above (NaN for a track not seen in the last pushed frame)
//   2. a frame is dropped iff its stamp or a robot coordinate is NaN
//   3. the kept frames share ONE grid: the bins of step 4 above, counted back from the newest kept frame (the anchor), nb and n_grid as
//      above; the robot's column is frames_kernel's
//   4. pedestrian j's frames are the kept ones where both its coordinates are non-NaN.  A bin holds the last sorted of them; an empty bin
//      between filled ones is interpolated between the nearest filled older and newer bin OF THAT TRACK by the formula of step 5 above
//      (x = nb-1-b with the shared nb); nothing is extrapolated in front of its oldest filled bin b_old(j), which may lie beyond F-1
//   5. the outputs are RIGHT-aligned in F rows: row p holds bin F-1-p, NaN in front (the layout of scene.py::pad_short_window, what
//      scene_kernel takes with first_frame); first_frame [N + 1], robot first: F - n_grid for the robot, F-1 - min(b_old(j), n_grid-1) for
//      pedestrian j, -1 for a pedestrian not seen in the anchor frame (absent now: its column NaN, the host refuses the build)
// One wavefront per episode, a lane per raw frame for the stamps and bins (LDS, shared by all tracks); a track's seen set over the 64
// lanes is one ballot word; then one lane per (track, row) finds the last sorted seen frame of its bin, or the two ends of its
// interpolation, reads the coordinates where they lie and writes its two doubles - every output element once, plain vector stores, a
// fixed order.  frames_kernel itself is untouched.
//
// track_frames_coast_kernel: track_frames_kernel for pedestrians who are not seen in the anchor frame (jmid_build_scene_stamped_coast;
// the device twin of scene.py::frame_table_tracks(max_coast=), in its operation order).  One lane per track scans its ballot word for
// its newest and oldest filled bin, b_new and b_old:
//   * seen in the anchor frame: everything as in track_frames_kernel, coast 0
//   * no filled bin, b_new > max_coast or b_new > n_grid-1: left out - first_frame -1, column and pose_now NaN, coast -1
//   * otherwise COASTED: the bins b >= b_new by rule 4 above (bin b_new is filled, so an empty bin behind it has both ends); the bins
//     b < b_new are y(b) = y(b_new) + (double)(b_new - b) * step, step = y(b_new) - y(b_new + 1) when the grid row b_new + 1 exists in
//     the track's window (b_new + 1 <= min(b_old, n_grid-1); real or interpolated), 0 otherwise - fp64, no FMA contraction;
//     first_frame by the same formula, pose_now = y(0), coast = b_new
// The (track, row) lanes of the bins < b_new evaluate rule 4 at b_new and b_new + 1 themselves: every output element is still written
// once, by one lane.  track_frames_kernel and frames_kernel are untouched.
//
// assemble_kernel: the device twin of scene.py::assemble_forecasts (mid_sim_wrapper.py:493-510, :444-454): one thread per
// (episode, pedestrian, kept sample) writes its (T + 1) x 2 doubles of forecasts [E, N, k, T+1, 2] and its double of logw [E, N, k].
// Copies and exact fp32 -> fp64 widenings only; plain vector stores, no atomics, a fixed order: bit-reproducible.  A track whose resident
// first_index is -1 (not in the scene) gets NaN in its forecast rows, the prepended pose included, and in its log-weight row.
#pragma once
#include "common.hpp"
#include "scene.hpp"

namespace jmid {

constexpr int FRM_MAX_R = 64;         // raw frames per episode: one lane each

struct FramesArgs {
    const double* stamps;         // [E, R]
    const double* human_xy;       // [E, R, N, 2]
    const double* robot_xy;       // [E, R, 2]
    const int* n_frames;          // [E] valid frames per episode (the first n_frames[e] of the R, oldest-pushed first), or null: all R
    double* o_human;              // [E, F, N, 2]
    double* o_robot;              // [E, F, 2]
    double* o_pose;               // [E, N, 2]
    int* o_n_grid;                // [E]   (-1: n_frames[e] outside 1..R, nothing else written for that episode)
    long long w;                  // round(time_step * 100) >= 1
    int E, N, R, F;
};

// t [R] fp64 | bin [R] int64 | x0, x1, x [F] fp64 | lo, hi [F] int
inline size_t frames_lds(int R, int F) { return (size_t)R * 16 + (size_t)F * (24 + 8); }

static __global__ __launch_bounds__(SCN_LANES) void frames_kernel(FramesArgs g) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char frm_lds_raw[];
    const int i = threadIdx.x, e = blockIdx.x;
    const int N = g.N, R = g.R, F = g.F, C = 2 * N + 2;
    double* t = reinterpret_cast<double*>(frm_lds_raw);       // [R] stamps
    long long* bin = reinterpret_cast<long long*>(t + R);     // [R] bin counted back from the newest stamp, -1 = dropped
    double* bx = reinterpret_cast<double*>(bin + R);          // [F, 3] x0, x1, x of an interpolated bin
    int* lo = reinterpret_cast<int*>(bx + 3 * F);             // [F] the frame a filled bin holds / the older end of an empty one
    int* hi = lo + F;                                         // [F] -1 for a filled bin / the newer end of an empty one
    const int n = g.n_frames ? g.n_frames[e] : R;
    if (n < 1 || n > R) {                                     // (uniform: the whole wavefront leaves)
        if (i == 0) g.o_n_grid[e] = -1;
        return;
    }
    const double* st = g.stamps + (size_t)e * R;
    const double* hum = g.human_xy + (size_t)e * R * N * 2;
    const double* rob = g.robot_xy + (size_t)e * R * 2;
    double* oh = g.o_human + (size_t)e * F * N * 2;
    double* orb = g.o_robot + (size_t)e * F * 2;
    // column c of raw frame r: the 2N human coordinates, then the robot's two (the frame table's column order)
    auto val = [&](int r, int c) -> double { return c < 2 * N ? hum[(size_t)r * 2 * N + c] : rob[r * 2 + (c - 2 * N)]; };
    // step 1
    for (int q = i; q < 2 * N; q += SCN_LANES) g.o_pose[(size_t)e * 2 * N + q] = hum[(size_t)(n - 1) * 2 * N + q];
    // step 2: frame by frame, the lanes over its columns; the mask is the same in every lane
    unsigned long long keep = 0;
    for (int r = 0; r < n; ++r) {
        bool bad = false;
        for (int c = i; c < C; c += SCN_LANES) {
            const double v = val(r, c);
            bad = bad || v != v;
        }
        if (i == 0) {
            const double s = st[r];
            bad = bad || s != s;
        }
        if (!__ballot(bad)) keep |= 1ull << r;
    }
    if (i < n) t[i] = st[i];
    __syncthreads();
    int n_grid = 0;
    long long nb = 0;
    if (keep) {
        // steps 3-4: the newest frame = the last one in (stamp, push index) order
        int last = -1;
        for (int j = 0; j < n; ++j)
            if (((keep >> j) & 1ull) && (last < 0 || t[j] >= t[last])) last = j;
        const long long ns_last = (long long)trunc(t[last] * 100.0);
        if (i < n) {
            long long b = -1;
            if ((keep >> i) & 1ull) {
                const long long a = ns_last - (long long)trunc(t[i] * 100.0);
                b = a / g.w;
                if (a % g.w != 0 && a < 0) --b;               // floor division (a >= 0 for sorted stamps; w >= 1)
            }
            bin[i] = b;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j)
            if (bin[j] + 1 > nb) nb = bin[j] + 1;
        n_grid = nb < (long long)F ? (int)nb : F;
        // step 5: one lane per needed bin finds its source frames
        if (i < n_grid) {
            const long long b = i;
            int hit = -1;
            long long bo = -1, bn = -1;                       // the nearest filled older / newer bin
            for (int j = 0; j < n; ++j) {
                const long long bj = bin[j];
                if (bj < 0) continue;
                if (bj == b && (hit < 0 || t[j] >= t[hit])) hit = j;
                if (bj > b && (bo < 0 || bj < bo)) bo = bj;
                if (bj < b && bj > bn) bn = bj;
            }
            if (hit >= 0) {
                lo[i] = hit;
                hi[i] = -1;
            } else {
                int jo = -1, jn = -1;                          // their last frames
                for (int j = 0; j < n; ++j) {
                    if (bin[j] == bo && (jo < 0 || t[j] >= t[jo])) jo = j;
                    if (bin[j] == bn && (jn < 0 || t[j] >= t[jn])) jn = j;
                }
                lo[i] = jo;
                hi[i] = jn;
                bx[i * 3] = (double)(nb - 1 - bo);
                bx[i * 3 + 1] = (double)(nb - 1 - bn);
                bx[i * 3 + 2] = (double)(nb - 1 - b);
            }
        }
    }
    __syncthreads();
    // step 6: grid row p holds bin n_grid-1-p; the rows behind the grid are zero
    for (int q = i; q < F * C; q += SCN_LANES) {
        const int p = q / C, c = q % C;
        double y = 0.0;
        if (p < n_grid) {
            const int b = n_grid - 1 - p;
            y = val(lo[b], c);
            if (hi[b] >= 0) {
                const double y1 = val(hi[b], c), x0 = bx[b * 3], x1 = bx[b * 3 + 1], x = bx[b * 3 + 2];
                const double slope = (y1 - y) / (x1 - x0);
                y = slope * (x - x0) + y;
            }
        }
        if (c < 2 * N) oh[(size_t)p * 2 * N + c] = y;
        else orb[p * 2 + (c - 2 * N)] = y;
    }
    if (i == 0) g.o_n_grid[e] = n_grid;
}

inline hipError_t launch_frames(const FramesArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(frames_kernel, dim3(g.E), dim3(SCN_LANES), frames_lds(g.R, g.F), st, g);
    return hipGetLastError();
}

// FramesArgs (o_human right-aligned: NaN in front, the newest frame in row F-1) and
struct TrackFramesArgs : FramesArgs {
    int* o_first;                 // [E, N + 1]   robot first; -1: a pedestrian not seen in the anchor frame
};

// the shared bins of step 3 and the seen sets of step 4 (column group N = the robot: the kept frames)
struct TrackFramesLds {
    double t[FRM_MAX_R];
    long long bin[FRM_MAX_R];
    unsigned long long seen[SCN_LANES];
};

static __global__ __launch_bounds__(SCN_LANES) void track_frames_kernel(TrackFramesArgs g) {
#pragma clang fp contract(off)
    __shared__ TrackFramesLds s;
    const int i = threadIdx.x, e = blockIdx.x;
    const int N = g.N, R = g.R, F = g.F;
    const int n = g.n_frames ? g.n_frames[e] : R;
    if (n < 1 || n > R) {                                     // (uniform: the whole wavefront leaves)
        if (i == 0) g.o_n_grid[e] = -1;
        return;
    }
    const double* st = g.stamps + (size_t)e * R;
    const double* hum = g.human_xy + (size_t)e * R * N * 2;
    const double* rob = g.robot_xy + (size_t)e * R * 2;
    double* oh = g.o_human + (size_t)e * F * N * 2;
    double* orb = g.o_robot + (size_t)e * F * 2;
    int* of = g.o_first + (size_t)e * (N + 1);
    const double nan = __builtin_nan("");
    // coordinate c (0, 1) of column group q in raw frame r: pedestrian q < N, the robot q == N
    auto val = [&](int r, int q, int c) -> double { return q < N ? hum[((size_t)r * N + q) * 2 + c] : rob[r * 2 + c]; };
    // step 1
    for (int q = i; q < 2 * N; q += SCN_LANES) g.o_pose[(size_t)e * 2 * N + q] = hum[(size_t)(n - 1) * 2 * N + q];
    // step 2: lane i holds raw frame i; one ballot word per column group says on which kept frames it is seen
    bool kept = false;
    if (i < n) {
        const double ts = st[i], rx = rob[i * 2], ry = rob[i * 2 + 1];
        kept = ts == ts && rx == rx && ry == ry;
        s.t[i] = ts;
    }
    const unsigned long long keep = __ballot(kept);
    for (int q = 0; q < N; ++q) {
        bool here = false;
        if (kept) {
            const double x = val(i, q, 0), y = val(i, q, 1);
            here = x == x && y == y;
        }
        const unsigned long long m = __ballot(here);
        if (i == 0) s.seen[q] = m;
    }
    if (i == 0) s.seen[N] = keep;
    __syncthreads();
    int n_grid = 0, last = -1;
    long long nb = 0;
    if (keep) {
        // step 3: the anchor = the last kept frame in (stamp, push index) order; every track shares its bins
        for (int j = 0; j < n; ++j)
            if (((keep >> j) & 1ull) && (last < 0 || s.t[j] >= s.t[last])) last = j;
        const long long ns_last = (long long)trunc(s.t[last] * 100.0);
        if (i < n) {
            long long b = -1;
            if (kept) {
                const long long a = ns_last - (long long)trunc(s.t[i] * 100.0);
                b = a / g.w;
                if (a % g.w != 0 && a < 0) --b;               // floor division (a >= 0 for sorted stamps; w >= 1)
            }
            s.bin[i] = b;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j)
            if (s.bin[j] + 1 > nb) nb = s.bin[j] + 1;
        n_grid = nb < (long long)F ? (int)nb : F;
    }
    // steps 4-5: one (column group, row) per lane and pass; row p holds bin F-1-p.  NaN: a row in front of the grid, a bin older than
    // the track's oldest filled one, a pedestrian not seen in the anchor frame
    for (int u = i; u < (N + 1) * F; u += SCN_LANES) {
        const int q = u / F, p = u % F;
        const long long b = F - 1 - p;
        const unsigned long long m = last < 0 ? 0ull : s.seen[q];
        double y[2] = {nan, nan};
        if (b < n_grid && ((m >> last) & 1ull)) {
            int hit = -1;
            long long bo = -1, bn = -1;                       // the track's nearest filled older / newer bin
            for (int j = 0; j < n; ++j) {
                if (!((m >> j) & 1ull)) continue;
                const long long bj = s.bin[j];
                if (bj == b && (hit < 0 || s.t[j] >= s.t[hit])) hit = j;
                if (bj > b && (bo < 0 || bj < bo)) bo = bj;
                if (bj < b && bj > bn) bn = bj;
            }
            if (hit >= 0) {
                y[0] = val(hit, q, 0);
                y[1] = val(hit, q, 1);
            } else if (bo >= 0 && bn >= 0) {                  // (bn: bin 0 holds the anchor; no bo: older than the track - NaN)
                int jo = -1, jn = -1;                         // their last frames
                for (int j = 0; j < n; ++j) {
                    if (!((m >> j) & 1ull)) continue;
                    if (s.bin[j] == bo && (jo < 0 || s.t[j] >= s.t[jo])) jo = j;
                    if (s.bin[j] == bn && (jn < 0 || s.t[j] >= s.t[jn])) jn = j;
                }
                const double x0 = (double)(nb - 1 - bo), x1 = (double)(nb - 1 - bn), x = (double)(nb - 1 - b);
                for (int c = 0; c < 2; ++c) {
                    const double y0 = val(jo, q, c), y1 = val(jn, q, c);
                    const double slope = (y1 - y0) / (x1 - x0);
                    y[c] = slope * (x - x0) + y0;
                }
            }
        }
        double* o = q < N ? oh + ((size_t)p * N + q) * 2 : orb + p * 2;
        o[0] = y[0];
        o[1] = y[1];
    }
    // first_frame: lane q for pedestrian q, lane N for the robot
    if (i <= N) {
        int f = -1;
        if (i == N) {
            f = F - n_grid;
        } else if (last >= 0 && ((s.seen[i] >> last) & 1ull)) {
            long long b_old = 0;
            for (int j = 0; j < n; ++j)
                if (((s.seen[i] >> j) & 1ull) && s.bin[j] > b_old) b_old = s.bin[j];
            f = F - 1 - (int)(b_old < (long long)(n_grid - 1) ? b_old : (long long)(n_grid - 1));
        }
        of[i == N ? 0 : i + 1] = f;
    }
    if (i == 0) g.o_n_grid[e] = n_grid;
}

inline hipError_t launch_track_frames(const TrackFramesArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(track_frames_kernel, dim3(g.E), dim3(SCN_LANES), 0, st, g);
    return hipGetLastError();
}

struct TrackCoastArgs : TrackFramesArgs {
    int* o_coast;                 // [E, N]   0: seen in the anchor frame; b_new: coasted over b_new bins; -1: left out
    int max_coast;                // 0 .. F-2
};

// TrackFramesLds and every track's newest filled bin (-1: no column) and min(oldest filled bin, n_grid-1); entry N = the robot
struct TrackCoastLds : TrackFramesLds {
    int b_new[SCN_LANES];
    int b_old[SCN_LANES];
};

// Rule 4 for one bin of one track (m: its seen set, q: its column group; tc: where the raw coordinates lie): the last sorted seen frame of
// bin b, or the interpolation between the nearest filled older and newer bin, or NaN where one of the two is missing
struct TrackCols {
    const double *hum, *rob;
    int N, n;
    long long nb;
};

static __device__ inline void track_bin_value(const TrackFramesLds& s, const TrackCols& tc, unsigned long long m, int q, long long b, double* y) {
#pragma clang fp contract(off)
    const int N = tc.N, n = tc.n;
    auto val = [&](int r, int c) -> double { return q < N ? tc.hum[((size_t)r * N + q) * 2 + c] : tc.rob[r * 2 + c]; };
    int hit = -1;
    long long bo = -1, bn = -1;                               // the track's nearest filled older / newer bin
    for (int j = 0; j < n; ++j) {
        if (!((m >> j) & 1ull)) continue;
        const long long bj = s.bin[j];
        if (bj == b && (hit < 0 || s.t[j] >= s.t[hit])) hit = j;
        if (bj > b && (bo < 0 || bj < bo)) bo = bj;
        if (bj < b && bj > bn) bn = bj;
    }
    y[0] = y[1] = __builtin_nan("");
    if (hit >= 0) {
        y[0] = val(hit, 0);
        y[1] = val(hit, 1);
    } else if (bo >= 0 && bn >= 0) {
        int jo = -1, jn = -1;                                 // their last frames
        for (int j = 0; j < n; ++j) {
            if (!((m >> j) & 1ull)) continue;
            if (s.bin[j] == bo && (jo < 0 || s.t[j] >= s.t[jo])) jo = j;
            if (s.bin[j] == bn && (jn < 0 || s.t[j] >= s.t[jn])) jn = j;
        }
        const double x0 = (double)(tc.nb - 1 - bo), x1 = (double)(tc.nb - 1 - bn), x = (double)(tc.nb - 1 - b);
        for (int c = 0; c < 2; ++c) {
            const double y0 = val(jo, c), y1 = val(jn, c);
            const double slope = (y1 - y0) / (x1 - x0);
            y[c] = slope * (x - x0) + y0;
        }
    }
}

static __global__ __launch_bounds__(SCN_LANES) void track_frames_coast_kernel(TrackCoastArgs g) {
#pragma clang fp contract(off)
    __shared__ TrackCoastLds s;
    const int i = threadIdx.x, e = blockIdx.x;
    const int N = g.N, R = g.R, F = g.F;
    const int n = g.n_frames ? g.n_frames[e] : R;
    if (n < 1 || n > R) {                                     // (uniform: the whole wavefront leaves)
        if (i == 0) g.o_n_grid[e] = -1;
        return;
    }
    const double* st = g.stamps + (size_t)e * R;
    const double* hum = g.human_xy + (size_t)e * R * N * 2;
    const double* rob = g.robot_xy + (size_t)e * R * 2;
    double* oh = g.o_human + (size_t)e * F * N * 2;
    double* orb = g.o_robot + (size_t)e * F * 2;
    // steps 2-3 of track_frames_kernel: lane i holds raw frame i; the kept frames, the seen sets, the anchor and the shared bins
    bool kept = false;
    if (i < n) {
        const double ts = st[i], rx = rob[i * 2], ry = rob[i * 2 + 1];
        kept = ts == ts && rx == rx && ry == ry;
        s.t[i] = ts;
    }
    const unsigned long long keep = __ballot(kept);
    for (int q = 0; q < N; ++q) {
        bool here = false;
        if (kept) {
            const double x = hum[((size_t)i * N + q) * 2], y = hum[((size_t)i * N + q) * 2 + 1];
            here = x == x && y == y;
        }
        const unsigned long long m = __ballot(here);
        if (i == 0) s.seen[q] = m;
    }
    if (i == 0) s.seen[N] = keep;
    __syncthreads();
    int n_grid = 0, last = -1;
    long long nb = 0;
    if (keep) {
        for (int j = 0; j < n; ++j)
            if (((keep >> j) & 1ull) && (last < 0 || s.t[j] >= s.t[last])) last = j;
        const long long ns_last = (long long)trunc(s.t[last] * 100.0);
        if (i < n) {
            long long b = -1;
            if (kept) {
                const long long a = ns_last - (long long)trunc(s.t[i] * 100.0);
                b = a / g.w;
                if (a % g.w != 0 && a < 0) --b;               // floor division (a >= 0 for sorted stamps; w >= 1)
            }
            s.bin[i] = b;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j)
            if (s.bin[j] + 1 > nb) nb = s.bin[j] + 1;
        n_grid = nb < (long long)F ? (int)nb : F;
    }
    // every track's newest and oldest filled bin, by the lane of its number: a column for a track seen in the anchor frame (b_new 0)
    // and for one whose newest bin is at most max_coast bins back and inside the window
    if (i <= N) {
        int bw = -1, bl = -1;
        if (last >= 0) {
            const unsigned long long m = s.seen[i];
            long long mn = -1, mx = -1;
            for (int j = 0; j < n; ++j) {
                if (!((m >> j) & 1ull)) continue;
                const long long bj = s.bin[j];
                if (mn < 0 || bj < mn) mn = bj;
                if (bj > mx) mx = bj;
            }
            const bool anchor = (m >> last) & 1ull;
            if (mn >= 0 && (anchor || (mn <= (long long)g.max_coast && mn <= (long long)(n_grid - 1)))) {
                bw = (int)mn;
                bl = (int)(mx < (long long)(n_grid - 1) ? mx : (long long)(n_grid - 1));
            }
        }
        s.b_new[i] = bw;
        s.b_old[i] = bl;
    }
    __syncthreads();
    // one (column group, row) per lane and pass; row p holds bin F-1-p.  NaN: a track without a column, a bin older than its oldest
    const TrackCols tc{hum, rob, N, n, nb};
    const double nan = __builtin_nan("");
    for (int u = i; u < (N + 1) * F; u += SCN_LANES) {
        const int q = u / F, p = u % F;
        const int b = F - 1 - p, bw = s.b_new[q], bl = s.b_old[q];
        const unsigned long long m = last < 0 ? 0ull : s.seen[q];
        double y[2] = {nan, nan};
        if (bw >= 0 && b <= bl) {
            if (b >= bw) {
                track_bin_value(s, tc, m, q, b, y);
            } else {
                double y0[2], y1[2];
                track_bin_value(s, tc, m, q, bw, y0);
                const bool moving = bw + 1 <= bl;             // (uniform per track: its lanes agree)
                if (moving) track_bin_value(s, tc, m, q, bw + 1, y1);
                for (int c = 0; c < 2; ++c) {
                    const double step = moving ? y0[c] - y1[c] : 0.0;
                    y[c] = y0[c] + (double)(bw - b) * step;
                }
            }
        }
        double* o = q < N ? oh + ((size_t)p * N + q) * 2 : orb + p * 2;
        o[0] = y[0];
        o[1] = y[1];
        // pose_now by the lane of the track's newest row: the last pushed frame for a track seen in the anchor frame, as track_frames_kernel
        // has it; the coasted position, or NaN, for the others
        if (q < N && p == F - 1) {
            const bool anchor = last >= 0 && ((m >> last) & 1ull);
            double* po = g.o_pose + ((size_t)e * N + q) * 2;
            po[0] = anchor ? hum[((size_t)(n - 1) * N + q) * 2] : y[0];
            po[1] = anchor ? hum[((size_t)(n - 1) * N + q) * 2 + 1] : y[1];
        }
    }
    // first_frame and coast: lane q for pedestrian q, lane N for the robot
    if (i <= N) {
        const int f = i == N ? F - n_grid : s.b_new[i] < 0 ? -1 : F - 1 - s.b_old[i];
        g.o_first[(size_t)e * (N + 1) + (i == N ? 0 : i + 1)] = f;
        if (i < N) g.o_coast[(size_t)e * N + i] = s.b_new[i];
    }
    if (i == 0) g.o_n_grid[e] = n_grid;
}

inline hipError_t launch_track_frames_coast(const TrackCoastArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(track_frames_coast_kernel, dim3(g.E), dim3(SCN_LANES), 0, st, g);
    return hipGetLastError();
}

struct AssembleArgs {
    const unsigned char* in_cluster;      // [E, N]
    const float* src;                     // k < K: sel [E, A, k, T, 2]; k == K: pos [E, K, A, T, 2]
    const float* logw_in;                 // k < K: [E, A, k]; k == K: unused
    const double* cv;                     // [E, N, T, 2]
    const double* pose;                   // pose_now of episode e at pose + e * pose_stride: [N, 2]
    double* forecasts;                    // [E, N, k, T+1, 2]
    double* logw;                         // [E, N, k]
    double logw_full;                     // k == K: log(1 / K), computed on the host
    size_t pose_stride;
    int E, N, A, k, T, full;
    const int* first_index;               // [E, N] the resident scene's, or null; -1: not in the scene, NaN rows
};

constexpr int ASM_THREADS = 256;

static __global__ __launch_bounds__(ASM_THREADS) void assemble_kernel(AssembleArgs g) {
    const size_t idx = (size_t)blockIdx.x * ASM_THREADS + threadIdx.x;
    const int N = g.N, A = g.A, k = g.k, T = g.T;
    if (idx >= (size_t)g.E * N * k) return;
    const int j = (int)(idx % k), n = (int)((idx / k) % N), e = (int)(idx / ((size_t)k * N));
    const unsigned char* inc = g.in_cluster + (size_t)e * N;
    double* o = g.forecasts + idx * (size_t)(T + 1) * 2;
    if (g.first_index && g.first_index[(size_t)e * N + n] < 0) {
        const double nan = __builtin_nan("");
        for (int q = 0; q < (T + 1) * 2; ++q) o[q] = nan;
        g.logw[idx] = nan;
        return;
    }
    const double* pose = g.pose + (size_t)e * g.pose_stride + (size_t)n * 2;
    o[0] = pose[0];
    o[1] = pose[1];
    int a = 0;                                                // rank by ascending track id
    for (int m = 0; m < n; ++m) a += inc[m] ? 1 : 0;
    if (inc[n] && a < A) {
        // (k == K: sample j is row j of pos; the host tail's transpose)
        const float* s = g.src + (g.full ? ((size_t)e * k + j) * A + a : ((size_t)e * A + a) * k + j) * (size_t)T * 2;
        for (int q = 0; q < T * 2; ++q) o[2 + q] = (double)s[q];
    } else {
        const double* s = g.cv + ((size_t)e * N + n) * (size_t)T * 2;
        for (int q = 0; q < T * 2; ++q) o[2 + q] = s[q];
    }
    g.logw[idx] = g.full ? g.logw_full : (double)g.logw_in[(size_t)e * A * k + j];      // the row of in-cluster rank 0: all rows are equal
}

inline hipError_t launch_assemble(const AssembleArgs& g, hipStream_t st) {
    const size_t total = (size_t)g.E * g.N * g.k;
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((total + ASM_THREADS - 1) / ASM_THREADS)), dim3(ASM_THREADS), 0, st, g);
    return hipGetLastError();
}

}  // namespace jmid

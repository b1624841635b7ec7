// The tail of a denoise step - concat3 (d -> d_mid), concat4 (d_mid -> d_low), output layer (d_low -> 2) - as ONE 2 x d map per
// (episode, agent) row and step (split-fp16 modes).
//
// The three layers are ConcatSquash layers y = (W x + b) * gate + bias with NO nonlinearity between them, and their gates and
// biases depend on the (episode, agent) row r and the denoise step s only, never on the token.  With g3, g4, go = sigmoid(hyp[r] +
// thyp[s]) and h3, h4, ho = hyp[r] + thyp[s] at the g3 / b3 / g4 / b4 / go / bo offsets of the hyper rows the whole tail is, exactly,
//     e[m, o] = sum_i Weff[r, s][o, i] X[m, i] + beff[r, s][o]                                      o = 0, 1
//     v[o, c]    = go[o] Wo[o, c] g4[c]                                    [2, d_low]
//     q[o, j]    = sum_c v[o, c] W4[c, j]                                  [2, d_mid]
//     u[o, j]    = q[o, j] g3[j]
//     Weff[o, i] = sum_j u[o, j] W3[j, i]                                  [2, d]
//     beff[o]    = sum_j q[o, j] (g3[j] b3[j] + h3[j]) + go[o] sum_c Wo[o, c] (g4[c] b4[c] + h4[c]) + go[o] bo[o] + ho[o]
// A chunk has K * T (240 at the benchmark's shape) times fewer rows than tokens: the table is built per chunk for all steps in exact
// fp32 (tail_fold_table_kernel: 0.66 MFLOP per (r, s)), and a step's launch reads the last LayerNorm's X_hi rows (X_hi + X_lo in
// F16X3, as that mode's concat3 does) once, takes two fp32 dot products per token and goes on with the sampler update and the next
// step's embedding exactly as out_ddim*_kernel does (elementwise.hpp).  Both tail GEMMs, their Y3 / Y4 planes and the fp16 rounding
// of Y3 are gone.
//
// Every table entry is computed by ONE sequence of operations whatever the launch (all steps of a chunk at once or one step at a
// time), and a token's e by ONE column-to-lane mapping and reduction order in both step kernels: the results do not depend on the
// chunk plan, the lanes or the kernel form.
#pragma once
#include <cfloat>

#include "common.hpp"
#include "elementwise.hpp"

namespace jmid {

// ------------------------------------------------------------------------------------------------ the table
constexpr int kTailG = 8;            // (row, step) pairs per workgroup: W4 / W3 are read once for all of them
constexpr int kTailMaxD = 512, kTailMaxMid = 256, kTailMaxLow = 128;      // shape limits of the kernels below (plan_step checks them)

struct TailTableArgs {
    const float *W3, *b3;    // [d_mid, d], [d_mid]      concat3._layer
    const float *W4, *b4;    // [d_low, d_mid], [d_low]  concat4._layer
    const float *Wo, *bo;    // [2, d_low], [2]          linear._layer
    const float* hyp;        // [R, hyp_ld] ctx part of the hyper nets, the chunk's (episode, agent) rows
    const float* thyp;       // [steps, hyp_ld] time part, first step of the table
    float* weff;             // [steps, R, 2, d]
    float* beff;             // [steps, R, 2]
    int steps, R, d, dmid, dlow, hyp_ld;
    int g3, b3o, g4, b4o, go, boo;       // offsets into a hyper row
    int* range_flag;
};

// One workgroup per kTailG consecutive (step, row) pairs; the 2 * kTailG rows of v, q / u stay in LDS as [k][pair * 2 + o], so a
// thread that owns a column of W4 / W3 reads them as broadcast 16-byte words.  Sums run over k32 tiles with a partial sum per tile
// (as gemm_f32_kernel's TSUM instance: the error grows with the number of tiles, not of terms).
static __global__ __launch_bounds__(256) void tail_fold_table_kernel(TailTableArgs a) {
    constexpr int G2 = 2 * kTailG;
    __shared__ __attribute__((aligned(16))) float s_v[kTailMaxLow][G2];
    __shared__ __attribute__((aligned(16))) float s_q[kTailMaxMid][G2];
    __shared__ __attribute__((aligned(16))) float s_u[kTailMaxMid][G2];
    __shared__ float s_t4[kTailG][kTailMaxLow];      // g4 b4 + h4
    __shared__ float s_t3[kTailG][kTailMaxMid];      // g3 b3 + h3
    const int tid = threadIdx.x;
    const long pairs = (long)a.steps * a.R;
    const long p0 = (long)blockIdx.x * kTailG;
    const auto hrow = [&](int g) { return a.hyp + (size_t)((p0 + g < pairs ? p0 + g : pairs - 1) % a.R) * a.hyp_ld; };
    const auto trow = [&](int g) { return a.thyp + (size_t)((p0 + g < pairs ? p0 + g : pairs - 1) / a.R) * a.hyp_ld; };
    bool bad = false;

    // v and the constant part of concat4's output
    for (int id = tid; id < kTailG * a.dlow; id += 256) {
        const int g = id / a.dlow, c = id - g * a.dlow;
        const float *hr = hrow(g), *th = trow(g);
        const float g4 = sigmoidf_(hr[a.g4 + c] + th[a.g4 + c]);
        s_t4[g][c] = g4 * a.b4[c] + (hr[a.b4o + c] + th[a.b4o + c]);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float go = sigmoidf_(hr[a.go + o] + th[a.go + o]);
            s_v[c][2 * g + o] = go * a.Wo[o * a.dlow + c] * g4;
        }
    }
    __syncthreads();

    // q = v W4: thread j owns column j of W4
    for (int j = tid; j < a.dmid; j += 256) {
        float acc[G2];
#pragma unroll
        for (int k = 0; k < G2; ++k) acc[k] = 0.f;
        for (int c0 = 0; c0 < a.dlow; c0 += 32) {
            float part[G2];
#pragma unroll
            for (int k = 0; k < G2; ++k) part[k] = 0.f;
            const int c1 = c0 + 32 < a.dlow ? c0 + 32 : a.dlow;
#pragma unroll 8
            for (int c = c0; c < c1; ++c) {
                const float w = a.W4[(size_t)c * a.dmid + j];
#pragma unroll
                for (int k4 = 0; k4 < G2; k4 += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&s_v[c][k4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) part[k4 + e] = fmaf(v[e], w, part[k4 + e]);
                }
            }
#pragma unroll
            for (int k = 0; k < G2; ++k) acc[k] += part[k];
        }
        const float b3 = a.b3[j];
        float u[G2];
#pragma unroll
        for (int g = 0; g < kTailG; ++g) {
            const float *hr = hrow(g), *th = trow(g);
            const float g3 = sigmoidf_(hr[a.g3 + j] + th[a.g3 + j]);
            s_t3[g][j] = g3 * b3 + (hr[a.b3o + j] + th[a.b3o + j]);
            u[2 * g] = acc[2 * g] * g3;
            u[2 * g + 1] = acc[2 * g + 1] * g3;
        }
#pragma unroll
        for (int k4 = 0; k4 < G2; k4 += 4) {
            *reinterpret_cast<f32x4*>(&s_q[j][k4]) = f32x4{acc[k4], acc[k4 + 1], acc[k4 + 2], acc[k4 + 3]};
            *reinterpret_cast<f32x4*>(&s_u[j][k4]) = f32x4{u[k4], u[k4 + 1], u[k4 + 2], u[k4 + 3]};
        }
    }
    __syncthreads();

    // beff: one thread per (pair, o)
    if (tid < G2 && p0 + (tid >> 1) < pairs) {
        const int g = tid >> 1, o = tid & 1;
        float sj = 0.f;
        for (int j0 = 0; j0 < a.dmid; j0 += 32) {
            float part = 0.f;
            const int j1 = j0 + 32 < a.dmid ? j0 + 32 : a.dmid;
            for (int j = j0; j < j1; ++j) part = fmaf(s_q[j][tid], s_t3[g][j], part);
            sj += part;
        }
        float sc = 0.f;
        for (int c0 = 0; c0 < a.dlow; c0 += 32) {
            float part = 0.f;
            const int c1 = c0 + 32 < a.dlow ? c0 + 32 : a.dlow;
            for (int c = c0; c < c1; ++c) part = fmaf(a.Wo[o * a.dlow + c], s_t4[g][c], part);
            sc += part;
        }
        const float *hr = hrow(g), *th = trow(g);
        const float go = sigmoidf_(hr[a.go + o] + th[a.go + o]);
        const float be = sj + go * sc + go * a.bo[o] + (hr[a.boo + o] + th[a.boo + o]);
        a.beff[(size_t)(p0 + g) * 2 + o] = be;
        bad |= !(fabsf(be) <= FLT_MAX);
    }

    // Weff = u W3: thread i owns columns i and i + 256 of W3
    {
        const int i0 = tid, i1 = tid + 256;
        const bool on0 = i0 < a.d, on1 = i1 < a.d;
        const float* w0p = a.W3 + (on0 ? i0 : 0);
        const float* w1p = a.W3 + (on1 ? i1 : 0);
        float acc0[G2], acc1[G2];
#pragma unroll
        for (int k = 0; k < G2; ++k) acc0[k] = acc1[k] = 0.f;
        for (int j0 = 0; j0 < a.dmid; j0 += 32) {
            float part0[G2], part1[G2];
#pragma unroll
            for (int k = 0; k < G2; ++k) part0[k] = part1[k] = 0.f;
            const int j1 = j0 + 32 < a.dmid ? j0 + 32 : a.dmid;
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const float w0 = w0p[(size_t)j * a.d], w1 = w1p[(size_t)j * a.d];
#pragma unroll
                for (int k4 = 0; k4 < G2; k4 += 4) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(&s_u[j][k4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        part0[k4 + e] = fmaf(u[e], w0, part0[k4 + e]);
                        part1[k4 + e] = fmaf(u[e], w1, part1[k4 + e]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < G2; ++k) {
                acc0[k] += part0[k];
                acc1[k] += part1[k];
            }
        }
#pragma unroll
        for (int k = 0; k < G2; ++k) {
            if (p0 + (k >> 1) >= pairs) break;
            float* row = a.weff + ((size_t)(p0 + (k >> 1)) * 2 + (k & 1)) * a.d;
            if (on0) {
                row[i0] = acc0[k];
                bad |= !(fabsf(acc0[k]) <= FLT_MAX);
            }
            if (on1) {
                row[i1] = acc1[k];
                bad |= !(fabsf(acc1[k]) <= FLT_MAX);
            }
        }
    }
    if (bad) atomicOr(a.range_flag, 1);      // a non-finite map: the call reports JMID_ERANGE
}

inline hipError_t launch_tail_fold_table(const TailTableArgs& a, hipStream_t st) {
    const long pairs = (long)a.steps * a.R;
    hipLaunchKernelGGL(tail_fold_table_kernel, dim3((unsigned)((pairs + kTailG - 1) / kTailG)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the step
struct TailFoldArgs {
    const half_t* Xh;       // [M, d] blocked panels (common.hpp::blk_index): the last LayerNorm's hi plane
    const half_t* Xl;       // its fp16 lo plane (F16X3: LO instances), else unused
    const float* weff;      // [R, 2, d] this step's maps
    const float* beff;      // [R, 2]
    int d;
};

// Lane l owns columns 8 l ... 8 l + 7 (d <= 512): one 16-byte chunk of the token's row in panel l / 4, so the four lanes of a panel
// read one whole 64-byte line between them and a wave-instruction fetches the token's d / 32 lines, 8 KB apart, complete.
struct TailMap {
    f32x4 w[2][2];          // Weff[o][8 l ... 8 l + 7]
    float b0, b1;
};
__device__ __forceinline__ void tail_fold_map(const TailFoldArgs& f, int ea, int lane, TailMap& t) {
    const bool on = lane * 8 < f.d;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const float* row = f.weff + ((size_t)ea * 2 + o) * f.d + lane * 8;
        t.w[o][0] = on ? *reinterpret_cast<const f32x4*>(row) : f32x4{0.f, 0.f, 0.f, 0.f};
        t.w[o][1] = on ? *reinterpret_cast<const f32x4*>(row + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    t.b0 = f.beff[(size_t)ea * 2];
    t.b1 = f.beff[(size_t)ea * 2 + 1];
}
__device__ __forceinline__ f16x8 tail_fold_load(const half_t* plane, int d, int m, int lane) {
    f16x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane * 8 < d) x = *reinterpret_cast<const f16x8*>(plane + blk_index(m, lane * 8, d));
    return x;
}
// THE two dot products of a token: eight fmaf per lane in column order, then the wave butterfly, then beff
template <bool LO>
__device__ __forceinline__ void tail_fold_dot(f16x8 xh, f16x8 xl, const TailMap& t, float& e0, float& e1) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = LO ? (float)xh[e] + (float)xl[e] : (float)xh[e];
        s0 = fmaf(v, t.w[0][e >> 2][e & 3], s0);
        s1 = fmaf(v, t.w[1][e >> 2][e & 3], s1);
    }
    e0 = wave_sum(s0) + t.b0;
    e1 = wave_sum(s1) + t.b1;
}
// the sampler update of one token (out_update's expressions): DDIM, or DDPM with this step's draw
__device__ __forceinline__ void tail_fold_update(const OutArgs& a, float e0, float e1, float x0, float x1, float z0, float z1,
                                                 float& xn0, float& xn1) {
    if (a.ddpm) {
        xn0 = a.c0 * (x0 - a.c1 * e0) + a.sigma * z0;
        xn1 = a.c0 * (x1 - a.c1 * e1) + a.sigma * z1;
    } else {
        const float p0 = (x0 - e0 * a.c_e) / a.c_x, p1 = (x1 - e1 * a.c_e) / a.c_x;
        xn0 = a.n_x * p0 + a.n_e * e0;
        xn1 = a.n_x * p1 + a.n_e * e1;
    }
}

// one wave per token (few tokens: one scene).  `a`: the sampler's part of OutArgs (x, e_out, the step's coefficients, z, rmap).
template <bool EMBED_NEXT, bool LO>
__global__ __launch_bounds__(256) void tail_fold_kernel(TailFoldArgs f, OutArgs a, EmbedArgs nxt) {
    args_now_each(f, a, nxt);
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const f16x8 xh = tail_fold_load(f.Xh, f.d, m, lane);
    const f16x8 xl = LO ? tail_fold_load(f.Xl, f.d, m, lane) : xh;
    TailMap t;
    tail_fold_map(f, a.rmap.ea(m), lane, t);
    const float x0 = a.e_out ? 0.f : a.x[2 * (size_t)m], x1 = a.e_out ? 0.f : a.x[2 * (size_t)m + 1];
    const float z0 = (a.ddpm && a.z) ? a.z[2 * (size_t)m] : 0.f, z1 = (a.ddpm && a.z) ? a.z[2 * (size_t)m + 1] : 0.f;
    float e0, e1;
    tail_fold_dot<LO>(xh, xl, t, e0, e1);
    float xn0 = 0.f, xn1 = 0.f;
    if (a.e_out) {
        if (lane == 0) {
            a.e_out[2 * (size_t)m] = e0;
            a.e_out[2 * (size_t)m + 1] = e1;
        }
    } else {
        tail_fold_update(a, e0, e1, x0, x1, z0, z1, xn0, xn1);
        if (lane == 0) {
            a.x[2 * (size_t)m] = xn0;
            a.x[2 * (size_t)m + 1] = xn1;
        }
    }
    if (EMBED_NEXT) embed_row(nxt, m, lane, xn0, xn1);
}

// One wave per piece of a trajectory (tpw consecutive tokens of one (episode, agent) row, a divisor of T): the map and the next
// embedding's gate / bias once per wave, the rows of up to 12 tokens requested before the first reduction (out_ddim_piece's shape).
template <bool EMBED_NEXT, bool LO>
__global__ __launch_bounds__(256) void tail_fold_traj_kernel(TailFoldArgs f, OutArgs a, EmbedArgs nxt, int tpw) {
    args_now_each(f, a, nxt);
    const int lane = threadIdx.x & 63;
    const int piece = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int m0 = piece * tpw;
    if (m0 >= a.M) return;
    const int t0 = a.rmap.t_of(m0), ea = a.rmap.ea(m0);
    EmbedCols c[2];
    const int j0 = lane * 4, j1 = lane * 4 + 256;
    if (EMBED_NEXT) {
        const float* hrow = nxt.hyp + (size_t)ea * nxt.hyp_ld;
        if (j0 < nxt.d) embed_cols(nxt, j0, hrow, c[0]);
        if (j1 < nxt.d) embed_cols(nxt, j1, hrow, c[1]);
    }
    TailMap t;
    tail_fold_map(f, ea, lane, t);
    for (int tb = 0; tb < tpw; tb += 12) {
        const int nb = tpw - tb < 12 ? tpw - tb : 12;
        f16x8 xh[12], xl[LO ? 12 : 1];
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int m = m0 + tb + (u < nb ? u : 0);
            xh[u] = tail_fold_load(f.Xh, f.d, m, lane);
            if (LO) xl[LO ? u : 0] = tail_fold_load(f.Xl, f.d, m, lane);
        }
        // lane u holds x (and the DDPM draw) of token u of the block
        const int mu = m0 + tb + (lane < nb ? lane : 0);
        const float xl0 = a.e_out ? 0.f : a.x[2 * (size_t)mu], xl1 = a.e_out ? 0.f : a.x[2 * (size_t)mu + 1];
        const float zl0 = (a.ddpm && a.z) ? a.z[2 * (size_t)mu] : 0.f, zl1 = (a.ddpm && a.z) ? a.z[2 * (size_t)mu + 1] : 0.f;
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            if (u >= nb) continue;
            const int m = m0 + tb + u;
            float e0, e1;
            tail_fold_dot<LO>(xh[u], LO ? xl[LO ? u : 0] : xh[u], t, e0, e1);
            float xn0 = 0.f, xn1 = 0.f;
            if (a.e_out) {
                if (lane == 0) {
                    a.e_out[2 * (size_t)m] = e0;
                    a.e_out[2 * (size_t)m + 1] = e1;
                }
            } else {
                tail_fold_update(a, e0, e1, __shfl(xl0, u, 64), __shfl(xl1, u, 64), __shfl(zl0, u, 64), __shfl(zl1, u, 64), xn0, xn1);
                if (lane == 0) {
                    a.x[2 * (size_t)m] = xn0;
                    a.x[2 * (size_t)m + 1] = xn1;
                }
            }
            if (EMBED_NEXT) {
                if (j0 < nxt.d) embed_store_cols(nxt, m, j0, t0 + tb + u, xn0, xn1, c[0]);
                if (j1 < nxt.d) embed_store_cols(nxt, m, j1, t0 + tb + u, xn0, xn1, c[1]);
            }
        }
    }
}

#ifdef JMID_DIAGNOSTICS
// fp32 row-major [rows, K] -> the hi (and lo) fp16 planes in the blocked panel layout, as the last LayerNorm leaves them
static __global__ void tail_split_rows_kernel(const float* in, half_t* hi, half_t* lo, int rows, int K) {
    const size_t n = (size_t)rows * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        half_t h, l;
        split_f32(in[i], h, l);
        const size_t o = blk_index((int)(i / K), (int)(i % K), K);
        hi[o] = h;
        if (lo) lo[o] = l;
    }
}
#endif

}  // namespace jmid

// Layer 0's Q / K / V^T operand planes without its in_proj GEMM (split-fp16 modes, JMID).
//
// The input of layer 0 is the embedding (elementwise.hpp::embed_store_cols)
//     X0[m, :] = (W1[:, 0] x0_m + W1[:, 1] x1_m + b1) * gate[r, s] + bias[r, s] + PE[t_m, :]
// with gate / bias depending on the (episode, agent) row r and the denoise step s only, so its image under the linear in_proj is
//     QKV0[m, :] = x0_m U[r, s, :] + x1_m V[r, s, :] + C[r, s, :] + Ppe[t_m, :]
//     U = Win (W1[:, 0] * gate)    V = Win (W1[:, 1] * gate)    C = Win (b1 * gate + bias)    Ppe = Win PE[t] + b_in
// A chunk has K * T (240 at the benchmark's shape) times fewer rows than tokens: the three coefficient rows per (row, step) go
// through in_proj once per chunk for all steps (qkv0_coef_kernel + the exact-fp32 GEMM with per-tile sums, gemm_f32.hpp), Ppe is
// made when the weights are finalized, and a step's launch only expands them: three FMAs and an add per element, a pure store
// stream (qkv0_expand_kernel).  The fp16 rounding of X0 in front of the GEMM is gone: the planes are closer to the fp32 net.
//
// Every element is computed by ONE expression (qkv0_value) whatever the launch shape, tokens per wave or channels per wave: the
// planes of a token do not depend on its chunk, lane or batch.
#pragma once
#include "common.hpp"
#include "gemm_f16x3.hpp"

namespace jmid {

// ------------------------------------------------------------------------------------------------ coefficient rows
struct Qkv0CoefArgs {
    const float* W1;     // [d, 2]   concat1._layer.weight
    const float* b1;     // [d]
    const float* hyp;    // [R, hyp_ld] ctx part of the hyper nets, the chunk's (episode, agent) rows
    const float* thyp;   // [steps, hyp_ld] time part, first step of the table
    float* coef;         // [steps, R, 3, d]
    int steps, R, d, hyp_ld, goff, boff;
    int* range_flag;
};

// one thread per (step, row, 4 channels): embed_cols' gate and bias, then the three rows in_proj is applied to
static __global__ __launch_bounds__(256) void qkv0_coef_kernel(Qkv0CoefArgs a) {
    const int d4 = a.d >> 2;
    const long total = (long)a.steps * a.R * d4;
    bool overflow = false;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % d4) * 4;
        const long sr = idx / d4;
        const int r = (int)(sr % a.R), s = (int)(sr / a.R);
        const float* hrow = a.hyp + (size_t)r * a.hyp_ld;
        const float* th = a.thyp + (size_t)s * a.hyp_ld;
        f32x4 u, v, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cc = j + e;
            const float gate = sigmoidf_(hrow[a.goff + cc] + th[a.goff + cc]);
            const float bias = hrow[a.boff + cc] + th[a.boff + cc];
            u[e] = a.W1[2 * cc] * gate;
            v[e] = a.W1[2 * cc + 1] * gate;
            c[e] = a.b1[cc] * gate + bias;
            overflow |= !(fabsf(u[e]) <= kHalfMax) || !(fabsf(v[e]) <= kHalfMax) || !(fabsf(c[e]) <= kHalfMax);
        }
        float* o = a.coef + (size_t)sr * 3 * a.d + j;
        *reinterpret_cast<f32x4*>(o) = u;
        *reinterpret_cast<f32x4*>(o + a.d) = v;
        *reinterpret_cast<f32x4*>(o + 2 * a.d) = c;
    }
    if (overflow) atomicOr(a.range_flag, 1);
}

// ------------------------------------------------------------------------------------------------ expansion
struct Qkv0Args {
    const float* x;      // [M, 2]
    const float* uvc;    // [R, 3, 3d] this step's U / V / C rows
    const float* ppe;    // [max_len, 3d]
    half_t *Qh, *Ql, *Kh, *Kl;     // row-major [M, d]
    half_t *Vth, *Vtl;             // [nseq][nhead][hd][Spad], keys in vt_key_pos order
    unsigned char *Q8l, *K8h, *K8l;      // bf8 images INSTEAD of the fp16 Q_lo / K_lo planes (F16MX at head_dim 128), or null
    int M, d, hd, S, Spad, nseq;
    float qscale;
    RowMap rmap;
    int* range_flag;
    int x2;              // V^T_lo is not read
    int tpw;             // Q / K part: tokens per wave, a divisor of T
    int qk_slabs;        // ... 256-column slabs of [Q | K]
    int qk_blocks;       // workgroups of the Q / K part; the V^T part follows
    int v_cpw;           // V^T part: channels per wave, a multiple of 4 that divides d
    int v_kblocks;       // ... 256-key blocks per sequence
    int v_same_row;      // T % 4 == 0 and S % 4 == 0: the four keys of a granule share their (episode, agent) row
};

// THE expression of an element of QKV0
__device__ __forceinline__ float qkv0_value(float x0, float x1, float u, float v, float c, float p) {
    return fmaf(x0, u, fmaf(x1, v, c)) + p;
}

// Q / K: lanes along channels.  A wave takes `tpw` consecutive tokens of one trajectory (one row of the table) and 256 columns of
// [Q | K], four per lane: the coefficients stay in registers, a token is 8-byte (fp16 x 4) and 4-byte (bf8 x 4) stores, 512 and
// 256 contiguous bytes per wave-instruction.
__device__ __forceinline__ void qkv0_expand_qk(const Qkv0Args& a, int wave, int lane) {
    const int piece = wave / a.qk_slabs, slab = wave - piece * a.qk_slabs;
    const int m0 = piece * a.tpw;
    const int j = slab * 256 + lane * 4;       // column of [Q | K]
    if (m0 >= a.M || j >= 2 * a.d) return;
    const int part = j >= a.d, nn = j - part * a.d, n3 = 3 * a.d;
    const int t0 = a.rmap.t_of(m0);
    const float* row = a.uvc + (size_t)a.rmap.ea(m0) * 3 * n3 + j;
    const f32x4 u = *reinterpret_cast<const f32x4*>(row);
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + n3);
    const f32x4 c = *reinterpret_cast<const f32x4*>(row + 2 * n3);
    const float qs = part == 0 ? a.qscale : 1.0f;
    unsigned amax16 = 0;
    for (int i = 0; i < a.tpw; ++i) {
        const int m = m0 + i;
        const float x0 = a.x[2 * (size_t)m], x1 = a.x[2 * (size_t)m + 1];
        const f32x4 p = *reinterpret_cast<const f32x4*>(a.ppe + (size_t)(t0 + i) * n3 + j);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = qkv0_value(x0, x1, u[e], v[e], c[e], p[e]);
            if (part == 0) o[e] *= qs;
        }
        const Split4 sp = split_f32x4(o[0], o[1], o[2], o[3], amax16);
        const size_t at = (size_t)m * a.d + nn;
        if (part == 0) {
            store_stream(reinterpret_cast<i32x2_s*>(a.Qh + at), sp.hi);
            if (a.Q8l) store_stream(reinterpret_cast<int*>(a.Q8l + at), bf8_of_f16x4(sp.lo[0], sp.lo[1]));
            else store_stream(reinterpret_cast<i32x2_s*>(a.Ql + at), sp.lo);
        } else {
            store_stream(reinterpret_cast<i32x2_s*>(a.Kh + at), sp.hi);
            if (a.K8h) {
                store_stream(reinterpret_cast<int*>(a.K8h + at), bf8_of_f16x4(sp.hi[0], sp.hi[1]));
                store_stream(reinterpret_cast<int*>(a.K8l + at), bf8_of_f16x4(sp.lo[0], sp.lo[1]));
            } else {
                store_stream(reinterpret_cast<i32x2_s*>(a.Kl + at), sp.lo);
            }
        }
    }
    if (split_range_exceeded(amax16)) atomicOr(a.range_flag, 1);
}

// V^T: lanes along keys.  A wave takes 256 consecutive keys of one sequence, four per lane (one 8-byte granule of a V^T row), and
// `v_cpw` channels: every store instruction writes a contiguous run of up to 512 bytes of one V^T row.  Keys past S inside the
// last granule are written as zeros (they are padding: they meet P = 0).
__device__ __forceinline__ void qkv0_expand_v(const Qkv0Args& a, int wave, int lane) {
    const int slabs = a.d / a.v_cpw;
    const int per_seq = a.v_kblocks * slabs;
    const int seq = wave / per_seq, rest = wave - seq * per_seq;
    const int kb = rest / slabs, slab = rest - kb * slabs;
    const int k0 = (kb * 64 + lane) * 4;
    if (seq >= a.nseq || k0 >= a.S) return;
    const int n3 = 3 * a.d, nh = a.d / a.hd;
    float x0[4], x1[4];
    const float *rowp[4], *pep[4];
    bool live[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        live[q] = k0 + q < a.S;
        const int m = seq * a.S + (live[q] ? k0 + q : k0);
        x0[q] = a.x[2 * (size_t)m];
        x1[q] = a.x[2 * (size_t)m + 1];
        rowp[q] = a.uvc + (size_t)a.rmap.ea(m) * 3 * n3 + 2 * a.d;
        pep[q] = a.ppe + (size_t)a.rmap.t_of(m) * n3 + 2 * a.d;
    }
    const size_t pos = vt_key_pos(k0);
    unsigned amax16 = 0;
    for (int cc = slab * a.v_cpw; cc < (slab + 1) * a.v_cpw; cc += 4) {
        f32x4 u[4], v[4], c[4], p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q == 0 || !a.v_same_row) {
                u[q] = *reinterpret_cast<const f32x4*>(rowp[q] + cc);
                v[q] = *reinterpret_cast<const f32x4*>(rowp[q] + n3 + cc);
                c[q] = *reinterpret_cast<const f32x4*>(rowp[q] + 2 * n3 + cc);
            } else {
                u[q] = u[0];
                v[q] = v[0];
                c[q] = c[0];
            }
            p[q] = *reinterpret_cast<const f32x4*>(pep[q] + cc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = live[q] ? qkv0_value(x0[q], x1[q], u[q][e], v[q][e], c[q][e], p[q][e]) : 0.f;
            const Split4 sp = split_f32x4(o[0], o[1], o[2], o[3], amax16);
            const int ch = cc + e, head = ch / a.hd, vc = ch - head * a.hd;
            const size_t at = (((size_t)seq * nh + head) * a.hd + vc) * a.Spad + pos;
            store_stream(reinterpret_cast<i32x2_s*>(a.Vth + at), sp.hi);
            if (!a.x2) store_stream(reinterpret_cast<i32x2_s*>(a.Vtl + at), sp.lo);
        }
    }
    if (split_range_exceeded(amax16)) atomicOr(a.range_flag, 1);
}

// four waves per workgroup; the first qk_blocks workgroups write Q / K, the others V^T
static __global__ __launch_bounds__(256) void qkv0_expand_kernel(Qkv0Args a) {
    args_now(a);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x < a.qk_blocks) qkv0_expand_qk(a, blockIdx.x * 4 + w, lane);
    else qkv0_expand_v(a, ((int)blockIdx.x - a.qk_blocks) * 4 + w, lane);
}

// The launch shape of a chunk: how many tokens / channels a wave takes - enough waves to fill the chip where the chunk has them.
// Nothing here changes a bit of the result.
inline void qkv0_plan(Qkv0Args& a, int T) {
    a.qk_slabs = (2 * a.d + 255) / 256;
    a.tpw = T;
    while (a.tpw > 1 && ((long)(a.M / a.tpw) * a.qk_slabs < 4096 || T % a.tpw != 0)) --a.tpw;
    a.qk_blocks = (int)(((long)(a.M / a.tpw) * a.qk_slabs + 3) / 4);
    a.v_kblocks = (a.S + 255) / 256;
    a.v_cpw = a.d % 16 == 0 ? 16 : 4;
    while (a.v_cpw > 4 && (long)a.nseq * a.v_kblocks * (a.d / a.v_cpw) < 4096) a.v_cpw >>= 1;
    a.v_same_row = T % 4 == 0 && a.S % 4 == 0;
}
inline hipError_t launch_qkv0_expand(const Qkv0Args& a, hipStream_t st) {
    const long v_waves = (long)a.nseq * a.v_kblocks * (a.d / a.v_cpw);
    const int blocks = a.qk_blocks + (int)((v_waves + 3) / 4);
    hipLaunchKernelGGL(qkv0_expand_kernel, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

#ifdef JMID_DIAGNOSTICS
// the planes of a layer's Q / K / V back as fp32 [M, 3d]: hi + lo, a bf8 image where it replaces a lo plane, Q without its scale
struct QkvReadArgs {
    const half_t *Qh, *Ql, *Kh, *Kl, *Vth, *Vtl;
    const unsigned char *Q8l, *K8l;
    float* out;
    size_t M;
    int d, hd, S, Spad, x2;
    float qscale;
    float* out_lo = nullptr;      // the two planes apart: out takes the hi planes, out_lo [M, 3d] the lo planes / their bf8 images (jmid_dbg_layer)
};
__device__ __forceinline__ float f32_of_bf8(unsigned char b) {
    return (float)__builtin_bit_cast(half_t, (unsigned short)((unsigned)b << 8));
}
static __global__ void qkv_planes_read_kernel(QkvReadArgs a) {
    const size_t n = a.M * a.d;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / a.d;
        const int c = (int)(i % a.d);
        const size_t seq = m / a.S, key = m % a.S;
        const int head = c / a.hd, vc = c % a.hd;
        const size_t at = ((seq * (a.d / a.hd) + head) * a.hd + vc) * a.Spad + (size_t)vt_key_pos((int)key);
        const float qh = (float)a.Qh[i], ql = a.Q8l ? f32_of_bf8(a.Q8l[i]) : (float)a.Ql[i];
        const float kh = (float)a.Kh[i], kl = a.K8l ? f32_of_bf8(a.K8l[i]) : (float)a.Kl[i];
        const float vh = (float)a.Vth[at], vl = a.x2 ? 0.f : (float)a.Vtl[at];
        float* o = a.out + m * 3 * a.d;
        if (a.out_lo) {
            float* ol = a.out_lo + m * 3 * a.d;
            o[c] = qh / a.qscale;
            ol[c] = ql / a.qscale;
            o[a.d + c] = kh;
            ol[a.d + c] = kl;
            o[2 * a.d + c] = vh;
            ol[2 * a.d + c] = vl;
        } else {
            o[c] = (qh + ql) / a.qscale;
            o[a.d + c] = kh + kl;
            o[2 * a.d + c] = vh + vl;
        }
    }
}
#endif

}  // namespace jmid

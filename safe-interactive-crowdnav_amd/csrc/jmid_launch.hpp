// Launch helpers shared by the planner and the diagnostics entry points: one GEMM / LayerNorm launch on the stream it is given (a
// lane's, or the handle's), bracketed by the profiling events of its kernel class.
#pragma once
#include "jmid_ctx.hpp"

namespace jmid_host {

template <int EPI>
int run_gemm(jmid_ctx* h, hipStream_t stream, int cls, const GemmArgs& g) {
    if (g.K % GEMM_BK != 0) return fail(h, JMID_EINVAL, "GEMM K must be a multiple of 32");
    ProfScope ps(h, cls, stream);
    HIPCHK(h, launch_gemm_f32<EPI>(g, stream));
    return 0;
}

// plan: launch_plan.hpp::plan_gemm for this launch's EPI, OUT, M, N, K in the call's GEMM mode (CallMode::gemm) - the planner's
// (StepPlan), or made on the spot by a diagnostics entry point; g.x2 is the call's as well (gemm_h_args)
template <int EPI, int OUT>
int run_gemm_h(jmid_ctx* h, hipStream_t stream, int cls, GemmHArgs& g, const GemmPlan& plan) {
    if (g.K % GEMMH_BK != 0) return fail(h, JMID_EINVAL, "GEMM K must be a multiple of 32");
    if (plan.mode == GM_MX && !g.W8) return fail(h, JMID_EINVAL, "GEMM planned for F16MX without the bf8 image of its weight");
    g.range_flag = h->range_flag;
    ProfScope ps(h, cls, stream);
    HIPCHK(h, (launch_gemm_h<EPI, OUT>(g, plan, stream)));
    return 0;
}

// out_proj / linear2 + residual + LayerNorm as ONE small launch, the row statistics exchanged between the workgroups of a row tile (gemm_small.hpp, OUT_LNX; F16MX at d_model 512)
// plan: plan_gemm(GM_MX, EPI_BIAS, OUT_LNX, ...) of this launch (GS_SMALL_64x64: one workgroup per CU, GS_SMALL_64x64_TWO: two)
inline int run_gemm_lnx_small(jmid_ctx* h, hipStream_t stream, int cls, GemmHArgs& g, const GemmPlan& plan) {
    g.range_flag = h->range_flag;
    if (++h->lnx_epoch == 0) h->lnx_epoch = 1;        // (0 is what the zeroed granules hold)
    g.ln_epoch = h->lnx_epoch;
    g.ln_polls = h->tune.lnx_polls;
    g.ln_withhold = h->tune.lnx_withhold;
    // the kernel is written for the F16MX operand set (byte lo plane of the residual stream, bf8 image of W_lo) only
    if (!(g.x2 && g.W8 && g.ln_xl8)) return fail(h, JMID_EINVAL, "one-launch GEMM + LayerNorm without the F16MX operand set");
    ProfScope ps(h, cls, stream);
    HIPCHK(h, (launch_gemm_small<EPI_BIAS, OUT_LNX>(g, plan, stream)));
    return 0;
}

// The operands of one fp32 GEMM: A [M, K] x a linear of the weight table [N, K] -> C [M, N].  The epilogue fields are the caller's.
inline GemmArgs gemm_args(const RowMap& rm, int M, const float* A, const LinearW& w, float* C, int N, int K) {
    GemmArgs g{};
    g.rmap = rm; g.M = M; g.N = N; g.K = K;
    g.A = A; g.lda = K; g.W = w.W; g.ldw = K; g.bias = w.bias; g.C = C; g.ldc = N;
    return g;
}

// The operands of one split-fp16 GEMM in mode m: A planes [M, K] x a linear of the weight table [N, K] - in JMID_PREC_F16MX with the fp8
// image of the weight's lo plane (the kernels that have no fp8 path ignore it).  The output and epilogue fields are the caller's.
inline GemmHArgs gemm_h_args(const CallMode& m, const RowMap& rm, int M, const half_t* Ahi, const half_t* Alo, const LinearW& w, int N, int K) {
    GemmHArgs g{};
    g.rmap = rm; g.M = M; g.N = N; g.K = K;
    g.Ahi = Ahi; g.Alo = Alo; g.Whi = w.split.hi; g.Wlo = w.split.lo; g.bias = w.bias;
    g.W8 = m.mx ? w.w8 : nullptr;
    g.x2 = m.x2;
    return g;
}

inline int run_add_ln(jmid_ctx* h, hipStream_t stream, float* X, const float* Y, const float* gm, const float* bt, int M, int d,
               half_t* Xh = nullptr, half_t* Xl = nullptr, bool mxv2 = false, int no_lo_out = 0) {
    ProfScope ps(h, KC_ADD_LN, stream);
    if (mxv2) {      // gemm_ln2_mx.hpp: byte lo plane, that file's summation order (d == 512); 4 rows per wave
        hipLaunchKernelGGL(add_ln2_kernel, dim3((M + 15) / 16), dim3(256), bystander_lds(h->tune.bystander_lds, add_ln2_kernel), stream, Y, gm, bt, M, 1e-5f,
                           Xh, reinterpret_cast<unsigned char*>(Xl), no_lo_out, h->range_flag);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    const int rows_per_block = 4;
    dim3 grid((M + rows_per_block - 1) / rows_per_block);
    const int vpl = (d + 255) / 256;
    const bool planes = Xh != nullptr;   // split-fp16 mode: the residual stream lives only in its planes
#define JMID_LN(V)                                                                                                    \
    if (planes) hipLaunchKernelGGL((add_ln_kernel<V, true>), grid, dim3(256), bystander_lds(h->tune.bystander_lds, add_ln_kernel<V, true>), stream, X, Y, gm, bt, M, d, 1e-5f, Xh, Xl); \
    else hipLaunchKernelGGL((add_ln_kernel<V, false>), grid, dim3(256), bystander_lds(h->tune.bystander_lds, add_ln_kernel<V, false>), stream, X, Y, gm, bt, M, d, 1e-5f, Xh, Xl);
    switch (vpl) {
        case 1: JMID_LN(1) break;
        case 2: JMID_LN(2) break;
        case 3:
        case 4: JMID_LN(4) break;
        default: return fail(h, JMID_EINVAL, "d_model too large for add_ln");
    }
#undef JMID_LN
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // namespace jmid_host

// The denoising loss of the reference on the device: DiffusionTraj.get_loss (MID/models/diffusion.py:448-476), reached through
// AutoEncoder.get_loss (MID/models/autoencoder.py:105-122) from MID.validation() (MID/mid.py:252-296) - the noise-prediction MSE at one
// timestep PER AGENT ROW.  A loss call is one net evaluation with K = 1, so a row r = e A + a is T consecutive tokens of the [E, A, T, 2]
// tensors and owns exactly one row of the hyper nets' ctx part.  Two kernels around that evaluation:
//
//   loss_prepare_kernel  x_t = c0[t_r] x0 + c1[t_r] e (diffusion.py:456-461: two rounded products, one rounded sum - the reference forms
//                        them as separate tensor ops) and hyp[r, :] += time_table[t_r, :].  The time part of the four ConcatSquash hyper
//                        nets is additive and every kernel of the net reads hyp[row] + thyp[step]: with the row's timestep folded into
//                        its hyp row and a zero row as thyp they compute (h + th) + 0, the bits of a per-row expression.  One place
//                        does not add the two parts first: the output layer's bias off the folded tail (out_update, elementwise.hpp:
//                        ((s + bo) gate + h) + th) - there the two entries stay out of hyp and go to a per-row array, OutArgs::tbo.
//   loss_reduce_kernel   per element d = e_theta - e and d d in fp32 (F.mse_loss(reduction="none")), summed per row in fp64 by one wave
//                        with a fixed lane -> element map and a fixed exchange tree; loss_total_kernel - one workgroup - then adds the
//                        real rows in (e, a) order.  No atomics: nothing depends on chunk sizes, lanes or launch geometry.
//
// A padded call (padded.hpp): the rows of padded agents keep their zero x, are left out of the sums and are NaN in the per-row output.
#pragma once
#include "common.hpp"

namespace jmid {

struct LossPrepareArgs {
    float* x;               // [R, T2]: x0 on entry, x_t on exit
    const float* e;         // [R, T2]
    const int* t;           // [R] timesteps, 1 .. n_t - 1 (checked on the host)
    const float *c0, *c1;   // [n_t] sqrt(alpha_bar), sqrt(1 - alpha_bar)
    float* hyp;             // [R, tot] ctx part of the hyper nets
    const float* ttab;      // [n_t, tot] time part per timestep
    const int* n_agents;    // [E] or null
    float* tbo;             // [R, 2] or null: the time part of the entries bo, bo + 1 goes here instead of into hyp (OutArgs::tbo)
    int R, A, T2, tot, bo;
};

// one workgroup per row
static __global__ __launch_bounds__(256) void loss_prepare_kernel(LossPrepareArgs g) {
    const int r = blockIdx.x;
    if (r >= g.R) return;
    const int tr = g.t[r];
    const bool real = !g.n_agents || r % g.A < g.n_agents[r / g.A];
    if (real) {
        const float c0 = g.c0[tr], c1 = g.c1[tr];
        for (int i = threadIdx.x; i < g.T2; i += 256) {
            const size_t at = (size_t)r * g.T2 + i;
            g.x[at] = __fadd_rn(__fmul_rn(c0, g.x[at]), __fmul_rn(c1, g.e[at]));
        }
    }
    float* hr = g.hyp + (size_t)r * g.tot;
    const float* tt = g.ttab + (size_t)tr * g.tot;
    for (int j = threadIdx.x; j < g.tot; j += 256) {
        if (g.tbo && (j == g.bo || j == g.bo + 1)) g.tbo[2 * (size_t)r + (j - g.bo)] = tt[j];
        else hr[j] = __fadd_rn(hr[j], tt[j]);
    }
}

struct LossReduceArgs {
    const float *e_theta, *e;   // [R, T2]
    const int* n_agents;        // [E] or null
    double* rows;               // [R] sum of squared errors per row, NaN for a padded row
    double* loss;               // [2] mean over the real rows' components, number of components
    int R, A, T2;
};

__device__ __forceinline__ bool loss_row_real(const LossReduceArgs& g, int r) { return !g.n_agents || r % g.A < g.n_agents[r / g.A]; }

// one wave per row: lane l takes the elements l, l + 64, ... in that order, then the xor tree 32, 16, 8, 4, 2, 1
static __global__ __launch_bounds__(256) void loss_reduce_kernel(LossReduceArgs g) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= g.R) return;
    if (!loss_row_real(g, r)) {
        if (lane == 0) g.rows[r] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    double s = 0.0;
    for (int i = lane; i < g.T2; i += 64) {
        const size_t at = (size_t)r * g.T2 + i;
        const float d = __fsub_rn(g.e_theta[at], g.e[at]);
        s += (double)__fmul_rn(d, d);
    }
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) g.rows[r] = s;
}

// ONE workgroup: thread i adds its block of consecutive rows in order, thread 0 the 256 partial sums in order
static __global__ __launch_bounds__(256) void loss_total_kernel(LossReduceArgs g) {
    __shared__ double part[256];
    __shared__ int real[256];
    const int per = (g.R + 255) / 256, r0 = (int)threadIdx.x * per, r1 = min(r0 + per, g.R);
    double s = 0.0;
    int n = 0;
    for (int r = r0; r < r1; ++r)
        if (loss_row_real(g, r)) {
            s += g.rows[r];
            ++n;
        }
    part[threadIdx.x] = s;
    real[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0, cnt = 0.0;
        for (int i = 0; i < 256; ++i) {
            tot += part[i];
            cnt += (double)real[i] * (double)g.T2;
        }
        g.loss[0] = tot / cnt;
        g.loss[1] = cnt;
    }
}

inline hipError_t launch_loss_prepare(const LossPrepareArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(loss_prepare_kernel, dim3(g.R), dim3(256), 0, st, g);
    return hipGetLastError();
}

inline hipError_t launch_loss_reduce(const LossReduceArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((g.R + 3) / 4), dim3(256), 0, st, g);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(256), 0, st, g);
    return hipGetLastError();
}

}  // namespace jmid

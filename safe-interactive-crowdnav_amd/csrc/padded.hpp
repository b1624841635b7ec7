// Padded scene batches: episodes of different agent counts in ONE call of the uniform shape [E, K A, T], A = the largest count.
// Row r = s A + a of episode e is REAL iff a < n_agents[e]; token j = r T + t of the episode's sequence is a VALID KEY iff its row is
// real (the reference's attn_mask: block-diagonal over scenes, padded agents excluded as keys - MID/models/diffusion.py:186-195,
// MID/dataset/preprocessing.py:36-89).  Attention is the only operation of the net that couples rows, so the mask words below are all
// the attention kernels need; everything else is row-wise, runs on the padding rows too and is thrown away (pad_fill_kernel).
#pragma once
#include "common.hpp"

namespace jmid {

__host__ __device__ __forceinline__ int mask_words_per_seq(int S) { return (S + 31) / 32; }

// One uint32 per (episode, 32-key tile): bit i of word w = key 32 w + i is valid; bits at or past S are 0.  All attention kernels
// walk the keys in 32-key tiles, so one word belongs to one tile.  Built on the device from the uploaded counts: a captured loop
// replays on the same words' memory with whatever counts the call at hand wrote there.
static __global__ __launch_bounds__(256) void mask_words_kernel(const int* n_agents, unsigned* words, int E, int A, int T, int S) {
    const int nw = mask_words_per_seq(S);
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * nw) return;
    const int e = idx / nw, w = idx - e * nw;
    const int n = n_agents[e];
    unsigned bits = 0;
    for (int i = 0; i < 32; ++i) {
        const int key = 32 * w + i;
        if (key < S && (key / T) % A < n) bits |= 1u << i;
    }
    words[idx] = bits;
}

// buf viewed as [E, R, A, L] floats: the rows of padded agents (a >= n_agents[e]) are set to `value` - 0 on the way in (x_T, ctx, p0:
// whatever the caller left there, NaN included, is never read), quiet NaN on the way out (a consumer that forgets n_agents sees it
// at once).  Real rows are not touched.
static __global__ __launch_bounds__(256) void pad_fill_kernel(float* buf, const int* n_agents, int E, int R, int A, int L, float value) {
    const size_t total = (size_t)E * R * A * L;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t row = idx / L;
        const int a = (int)(row % A), e = (int)(row / ((size_t)R * A));
        if (a >= n_agents[e]) buf[idx] = value;
    }
}

inline hipError_t launch_mask_words(const int* n_agents, unsigned* words, int E, int A, int T, int S, hipStream_t st) {
    const int n = E * mask_words_per_seq(S);
    hipLaunchKernelGGL(mask_words_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n_agents, words, E, A, T, S);
    return hipGetLastError();
}
inline hipError_t launch_pad_fill(float* buf, const int* n_agents, int E, int R, int A, int L, float value, hipStream_t st) {
    const size_t total = (size_t)E * R * A * L;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(pad_fill_kernel, dim3(blocks), dim3(256), 0, st, buf, n_agents, E, R, A, L, value);
    return hipGetLastError();
}

}  // namespace jmid

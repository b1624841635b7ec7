// Seeded noise on the device: x_T and the per-step DDPM z as a pure function of (seed, episode id, draw, element).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) as a counter-based generator:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (q, episode_id, draw, 0)          q = idx / 4, idx the row-major element index inside the episode's [rows, T, 2] tensor
// The four output words of block q give the elements 4q .. 4q + 3 of the episode (the last block of an episode may be partly used: rows * T * 2
// is even, so it holds two or four).  draw 0 is x_T, draw i + 1 the z of step-table entry i.  Nothing else enters: an episode's values do
// not depend on the batch, chunk, lane or rank it is computed in.
//
// Normals: Box-Muller per word pair, (w0, w1) -> elements 4q, 4q + 1 and (w2, w3) -> 4q + 2, 4q + 3, evaluated in fp64 and rounded once:
//   u1 = (a + 1) * 2^-32 in (0, 1],  u2 = b * 2^-32 in [0, 1),  r = sqrt(-2 ln u1),  (r cos(2 pi u2), r sin(2 pi u2))
// with 2 pi the fp64 constant 6.283185307179586 and every product rounded on its own (no FMA contraction, as scene.hpp): the host twin
// (noise.py) evaluates the same expression in NumPy, and the two agree bit for bit except where the fp64 result lies within the libraries'
// last-place difference of an fp32 rounding boundary (about 1e-8 of the values).  |z| <= sqrt(64 ln 2) = 6.66.
//
// One thread per block of four outputs, vector stores where the destination allows them.  The kernel is memory-bound and tiny next to a
// denoise step.
#pragma once
#include "common.hpp"

namespace jmid {

struct NoiseArgs {
    const unsigned* ids;     // [E] episode ids (device)
    float* out;              // [E, n] normals, or null
    unsigned* words;         // [E, n] raw words, or null (diagnostics)
    unsigned long long n;    // elements per episode: rows * T * 2
    unsigned key0, key1;     // the seed's low and high word
    unsigned draw;
    int E;
    int vec;                 // widest store the destination's alignment and n allow: 4, 2 or 1 floats
};

__host__ __device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* w) {
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__host__ __device__ inline void box_muller(unsigned a, unsigned b, float* z) {
#pragma clang fp contract(off)
    const double u1 = ((double)a + 1.0) * 0x1p-32, u2 = (double)b * 0x1p-32;
    const double r = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
    z[0] = (float)(r * cos(th));
    z[1] = (float)(r * sin(th));
}

static __global__ __launch_bounds__(256) void noise_fill_kernel(NoiseArgs g) {
    const unsigned long long nq = (g.n + 3) / 4;
    const unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    for (int e = blockIdx.y; e < g.E; e += gridDim.y) {
        unsigned w[4];
        philox4x32_10((unsigned)q, g.ids[e], g.draw, 0u, g.key0, g.key1, w);
        const unsigned long long i0 = 4 * q, left = g.n - i0;          // left >= 1
        const size_t base = (size_t)e * g.n + i0;
        if (g.words) {
            for (int j = 0; j < 4; ++j)
                if ((unsigned long long)j < left) g.words[base + j] = w[j];
        }
        if (!g.out) continue;
        float z[4];
        box_muller(w[0], w[1], z);
        box_muller(w[2], w[3], z + 2);
        if (g.vec == 4 && left >= 4) {
            *reinterpret_cast<float4*>(g.out + base) = make_float4(z[0], z[1], z[2], z[3]);
        } else if (g.vec >= 2 && left >= 2) {
            *reinterpret_cast<float2*>(g.out + base) = make_float2(z[0], z[1]);
            if (left >= 4) *reinterpret_cast<float2*>(g.out + base + 2) = make_float2(z[2], z[3]);
            else if (left == 3) g.out[base + 2] = z[2];
        } else {
            for (int j = 0; j < 4; ++j)
                if ((unsigned long long)j < left) g.out[base + j] = z[j];
        }
    }
}

// The padded form (padded.hpp): episode e draws exactly what it draws alone - its COMPACT tensor [K * n_e, T, 2], n_e = n_agents[e], with
// idx = ((s * n_e + a) * T + t) * 2 + c and the counter (idx / 4, id, draw, 0) - and the value lands in padded row s * A + a of
// out [E, K * A, T, 2].  One thread per Philox block of the compact tensor, as above; the block's four elements may lie in two padded
// rows, so each word pair goes to its own destination (T * 2 is even: a pair never straddles a row, and a compact tensor ends on a pair).
// Padded rows are not written (the caller's pad_fill_kernel decides what they hold).
struct NoisePaddedArgs {
    const unsigned* ids;     // [E] episode ids (device)
    const int* n_agents;     // [E] counts (device), 1 .. A
    float* out;              // [E, K * A, T, 2]
    unsigned key0, key1;
    unsigned draw;
    int E, A, K, T;
    int vec;                 // 2: out is 8-byte aligned, float2 stores; 1: scalar stores
};

static __global__ __launch_bounds__(256) void noise_fill_padded_kernel(NoisePaddedArgs g) {
    const unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long L = (unsigned long long)g.T * 2;
    for (int e = blockIdx.y; e < g.E; e += gridDim.y) {
        const int ne = min(max(g.n_agents[e], 0), g.A);          // (the host has checked 1 .. A; a count outside could write out of bounds)
        const unsigned long long n = (unsigned long long)g.K * ne * L;
        if (4 * q >= n) continue;
        unsigned w[4];
        philox4x32_10((unsigned)q, g.ids[e], g.draw, 0u, g.key0, g.key1, w);
        float* oe = g.out + (size_t)e * g.K * g.A * L;
        for (int p = 0; p < 2; ++p) {
            const unsigned long long idx = 4 * q + 2 * p;
            if (idx >= n) break;
            float z[2];
            box_muller(w[2 * p], w[2 * p + 1], z);
            const unsigned long long r = idx / L, rem = idx - r * L, s = r / ne, a = r - s * ne;
            float* o = oe + (s * g.A + a) * L + rem;
            if (g.vec == 2) *reinterpret_cast<float2*>(o) = make_float2(z[0], z[1]);
            else o[0] = z[0], o[1] = z[1];
        }
    }
}

inline hipError_t launch_noise_padded(NoisePaddedArgs g, hipStream_t stream) {
    const unsigned long long nq = ((unsigned long long)g.K * g.A * g.T * 2 + 3) / 4;       // of the largest count an episode can have
    g.vec = reinterpret_cast<uintptr_t>(g.out) % 8 == 0 ? 2 : 1;
    const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)std::min(g.E, 65535));
    hipLaunchKernelGGL(noise_fill_padded_kernel, grid, dim3(256), 0, stream, g);
    return hipGetLastError();
}

// the limits of the addressing: the block index is one 32-bit counter word, the launch grid 2^31 - 1 workgroups
inline bool noise_fits(unsigned long long n) { return (n + 3) / 4 <= 0x100000000ull && ((n + 3) / 4 + 255) / 256 <= 0x7fffffffull; }

inline hipError_t launch_noise(NoiseArgs g, hipStream_t stream) {
    const unsigned long long nq = (g.n + 3) / 4;
    // float4 stores need every episode's base 16-byte aligned (n a multiple of 4), float2 stores an 8-byte aligned destination (n is even
    // for [rows, T, 2]; an odd n or a 4-byte aligned pointer takes scalar stores)
    const uintptr_t p = reinterpret_cast<uintptr_t>(g.out);
    g.vec = (g.n % 4 == 0 && p % 16 == 0) ? 4 : (g.n % 2 == 0 && p % 8 == 0) ? 2 : 1;
    const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)std::min(g.E, 65535));
    hipLaunchKernelGGL(noise_fill_kernel, grid, dim3(256), 0, stream, g);
    return hipGetLastError();
}

}  // namespace jmid

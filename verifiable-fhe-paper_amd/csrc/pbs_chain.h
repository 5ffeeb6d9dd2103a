// The pieces of a bootstrap chain that every one-workgroup-per-ciphertext kernel shares: the mod switch, the rotated coefficient and the
// two negacyclic transforms in LDS (two stages per pass, one __syncthreads() per pass).  One statement of them for pbs_batch.hip (one key
// set per launch) and pbs_keyring.hip (a key set per workgroup), as keygen_streams.h is for the generators: the same canonical-in,
// canonical-out field operations in the same order, so the words of the two kernels are the same.
#pragma once
#include <cstddef>

#include "gl.h"

namespace vpbs {
using gl::u64;

constexpr size_t PBS_LDS_BUDGET = 160 * 1024;   // what one workgroup may declare on gfx950

// rotation amount in [0, 2N]: top log2(2N) bits of the mask, rounded with the next bit (mod.rs:85-106); as tfhe.hip
__device__ __forceinline__ unsigned pb_mod_switch(u64 mask, unsigned log_n_ring) {
    const unsigned log2n = log_n_ring + 1;
    return (unsigned)(mask >> (64 - log2n)) + (unsigned)((mask >> (64 - log2n - 1)) & 1);
}
// coefficient i of poly * X^shift mod X^N + 1, 0 <= shift <= 2N; as tfhe.hip
__device__ __forceinline__ u64 pb_rotated_coeff(const u64* poly, unsigned n, unsigned shift, unsigned i) {
    const unsigned src = (i + 2 * n - shift) & (2 * n - 1);
    const u64 c = poly[src & (n - 1)];
    return src >= n ? gl::neg(c) : c;
}

// forward negacyclic NTT (crypto/poly.rs:9-34) of `cnt` polynomials back to back in LDS; ends behind a barrier
template <unsigned T>
__device__ __forceinline__ void pb_forward(u64* t, unsigned log_n, unsigned cnt, const u64* __restrict__ roots) {
    const unsigned n = 1u << log_n;
    unsigned m = 1, stages = log_n;
    while (stages >= 2) {   // stages m and 2m on the points j, j + h, j + len, j + len + h
        const unsigned len = n / (2 * m), h = len >> 1, log_h = stages - 2;
        for (unsigned q = threadIdx.x; q < cnt * (n >> 2); q += T) {
            const unsigned poly = q >> (log_n - 2), qq = q & ((n >> 2) - 1);
            const unsigned i = qq >> log_h, off = qq & (h - 1);
            u64* p = t + (size_t)poly * n + 2 * i * len + off;
            const u64 x0 = p[0], x1 = p[h], x2 = p[len], x3 = p[len + h];
            const u64 w = roots[m + i], w0 = roots[2 * m + 2 * i], w1 = roots[2 * m + 2 * i + 1];
            const u64 v2 = gl::mul(x2, w), v3 = gl::mul(x3, w);
            const u64 a0 = gl::add(x0, v2), a2 = gl::sub(x0, v2), a1 = gl::add(x1, v3), a3 = gl::sub(x1, v3);
            const u64 u1 = gl::mul(a1, w0), u3 = gl::mul(a3, w1);
            p[0] = gl::add(a0, u1);
            p[h] = gl::sub(a0, u1);
            p[len] = gl::add(a2, u3);
            p[len + h] = gl::sub(a2, u3);
        }
        __syncthreads();
        m <<= 2;
        stages -= 2;
    }
    if (stages == 1) {   // the last stage alone (odd log_n): m = n / 2, neighbours
        for (unsigned k = threadIdx.x; k < cnt * (n >> 1); k += T) {
            const unsigned poly = k >> (log_n - 1), i = k & ((n >> 1) - 1);
            u64* p = t + (size_t)poly * n + 2 * i;
            const u64 u = p[0], v = gl::mul(p[1], roots[m + i]);
            p[0] = gl::add(u, v);
            p[1] = gl::sub(u, v);
        }
        __syncthreads();
    }
}

// Inverse transform (crypto/poly.rs:36-64) of the `cnt` polynomials of t, in place; the LAST pass multiplies by N^-1 and hands each point
// to `finish(index in [cnt][N], value)` instead of storing it (the CMUX add into the accumulator).  Ends behind a barrier.
template <unsigned T, class Finish>
__device__ __forceinline__ void pb_inverse(u64* t, unsigned log_n, unsigned cnt, const u64* __restrict__ invroots, u64 ninv, Finish finish) {
    const unsigned n = 1u << log_n;
    unsigned m = n >> 1, stages = log_n, log_len = 0;
    while (stages >= 2) {   // stages m and m / 2 on the points j, j + len, j + 2 len, j + 3 len
        const unsigned len = 1u << log_len, m2 = m >> 1;
        const bool fin = stages == 2;
        for (unsigned q = threadIdx.x; q < cnt * (n >> 2); q += T) {
            const unsigned poly = q >> (log_n - 2), qq = q & ((n >> 2) - 1);
            const unsigned i2 = qq >> log_len, off = qq & (len - 1);
            const unsigned base = poly * n + 4 * i2 * len + off;
            u64* p = t + base;
            const u64 x0 = p[0], x1 = p[len], x2 = p[2 * len], x3 = p[3 * len];
            const u64 w0 = invroots[m + 2 * i2], w1 = invroots[m + 2 * i2 + 1], w = invroots[m2 + i2];
            const u64 a0 = gl::add(x0, x1), a1 = gl::mul(gl::sub(x0, x1), w0);
            const u64 a2 = gl::add(x2, x3), a3 = gl::mul(gl::sub(x2, x3), w1);
            const u64 y0 = gl::add(a0, a2), y2 = gl::mul(gl::sub(a0, a2), w);
            const u64 y1 = gl::add(a1, a3), y3 = gl::mul(gl::sub(a1, a3), w);
            if (fin) {
                finish(base, gl::mul(y0, ninv));
                finish(base + len, gl::mul(y1, ninv));
                finish(base + 2 * len, gl::mul(y2, ninv));
                finish(base + 3 * len, gl::mul(y3, ninv));
            } else {
                p[0] = y0;
                p[len] = y1;
                p[2 * len] = y2;
                p[3 * len] = y3;
            }
        }
        __syncthreads();
        m >>= 2;
        stages -= 2;
        log_len += 2;
    }
    if (stages == 1) {   // the last stage alone (odd log_n): m = 1, halves
        const unsigned len = n >> 1;
        const u64 w = invroots[1];
        for (unsigned k = threadIdx.x; k < cnt * len; k += T) {
            const unsigned poly = k >> (log_n - 1), i = k & (len - 1);
            const unsigned base = poly * n + i;
            const u64 u = t[base], v = t[base + len];
            finish(base, gl::mul(gl::add(u, v), ninv));
            finish(base + len, gl::mul(gl::mul(gl::sub(u, v), w), ninv));
        }
        __syncthreads();
    }
}
}  // namespace vpbs

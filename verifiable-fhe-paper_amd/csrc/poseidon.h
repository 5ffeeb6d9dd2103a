// Poseidon permutation over Goldilocks (width 12, rate 8, x^7, 8 full + 22 partial rounds): product code, host +
// gfx950.  Replaces plonky2 0.2.0 hash/poseidon.rs `Poseidon::poseidon` / hash/poseidon_goldilocks.rs as used by
// PoseidonHash (leaf hashing, two_to_one, Challenger); native use in the reference:
// /root/reference/src/vtfhe/ivc_based_vpbs.rs:73.
//
// Arithmetic form (device): the state is kept as arbitrary u64 residues between rounds.  The MDS layer
// (circulant [17,15,41,16,2,28,13,13,39,18,34,20] + diag[8,0..]) is evaluated on the 32-bit halves of the state with
// v_mad_u64_u32 accumulators (all coefficients are inline constants <= 41), the next round's constants are the
// accumulators' initial values (the constant layer costs nothing), and one 96-bit -> 64-bit fold per element ends
// the round.  No MFMA: this is 64-bit modular integer work.
#pragma once
#include "gl.h"

namespace poseidon {
using gl::u32;
using gl::u64;

constexpr int WIDTH = 12, RATE = 8, N_ROUNDS = 30, HALF_FULL = 4, N_PARTIAL = 22;

// 360 round constants + 12 zeros: the constants "after the last round".  The last MDS layer adds nothing; until round 9 it ran as a round like
// the others and loaded this zero block (no select in front of the scalar loads' first use), now it is last_rows and reads no constants.
static const u64 RC_HOST[372] = {
#include "poseidon_constants.inc"
};
#if defined(__HIPCC__)
static __constant__ u64 RC_DEV[372] = {
#include "poseidon_constants.inc"
};
#endif

#include "poseidon_partial_groups.inc"
static const PartialGroup PG_HOST[7] = POSEIDON_PARTIAL_GROUPS_INIT;
#if defined(__HIPCC__)
static __constant__ PartialGroup PG_DEV[7] = POSEIDON_PARTIAL_GROUPS_INIT;
#endif
GL_HD const PartialGroup& partial_group(int g) {
#if defined(__HIP_DEVICE_COMPILE__)
    return PG_DEV[g];
#else
    return PG_HOST[g];
#endif
}

GL_HD u64 rc(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return RC_DEV[i];
#else
    return RC_HOST[i];
#endif
}

GL_HD u64 sbox(u64 x) {
    const u64 x2 = gl::mul_nc(x, x);
    const u64 x4 = gl::mul_nc(x2, x2);
    const u64 x3 = gl::mul_nc(x2, x);
    return gl::mul_nc(x3, x4);
}

// two S-boxes with their multiplication chains interleaved (hides the dependent-instruction latency of the asm blocks)
GL_HD void sbox2(u64& x, u64& y) {
    u64 x2, y2, x3, y3, x4, y4;
    gl::mul2_nc(x, x, y, y, x2, y2);
    gl::mul2_nc(x2, x2, y2, y2, x4, y4);
    gl::mul2_nc(x2, x, y2, y, x3, y3);
    gl::mul2_nc(x3, x4, y3, y4, x, y);
}

// S-box with x^3 and x^4 computed side by side (three dependent multiplications deep instead of four)
GL_HD u64 sbox_ilp(u64 x) {
    const u64 x2 = gl::mul_nc(x, x);
    u64 x3, x4;
    gl::mul2_nc(x2, x, x2, x2, x3, x4);
    return gl::mul_nc(x3, x4);
}

// acc_lo + acc_hi * 2^32 folded to a u64 residue with 2^64 = 2^32 - 1.  What it rests on: T = (acc_hi >> 32) (2^32 - 1) + acc_lo < 2^64 (the MDS and
// group rows stay below 2^59, the closing group's below 2^62: the table in DESIGN.md section 4)
GL_HD u64 fold96(u64 acc_lo, u64 acc_hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    // acc_lo + (hi_lo + hi_hi 2^32) 2^32 = acc_lo + hi_hi 2^64 + hi_lo 2^32: T = hi_hi (2^32 - 1) + acc_lo as ONE v_mad_u64_u32 (below 2^59:
    // no carry), then hi_lo joins T's high word; that carry selects the single +(2^32 - 1) correction (the wrapped value is below T, so the
    // corrected sum cannot wrap again).  The correction is one more multiply-add, t (2^32 - 1) + T with t = carry ? 1 : 0, into the aligned pair of
    // the 64-bit result: 4 VALU (round 8; 5 with the select of 0 / -1 and a 64-bit addition, round 5; 7 before that: the sum L was formed first,
    // with a carry into H and a move to pair it).
    u64 r;
    // (scratch through gl.h's names: a translation unit built with GL_ASM_SCRATCH_LOW -- quotient.hip, permutation.hip -- keeps its register
    // budget; with v80 / v81 / v86 spelled out here those kernels were pushed to 87 VGPRs whatever the setting: ADVICE r05)
    asm("v_mad_u64_u32 " GL_P01 ", vcc, %3, -1, %1\n\t"
        "v_add_co_u32_e32 " GL_R1 ", vcc, " GL_R1 ", %2\n\t"
        GL_SEL01(GL_R6, "vcc")
        GL_ADD_EPS_IF("%0", GL_R6, GL_P01)
        : "=v"(r)
        : "v"(acc_lo), "v"((u32)acc_hi), "v"((u32)(acc_hi >> 32))
        : GL_R0, GL_R1, GL_R6, "vcc");
    return r;
#else
    const u64 L = acc_lo + (acc_hi << 32);
    const u64 H = (acc_hi >> 32) + (L < acc_lo ? 1 : 0);
    const u64 t1 = (H << 32) - H;
    u64 v = L + t1;
    if (v < t1) v += gl::EPS;
    return v;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// One row of the MDS layer as ONE block of 24 multiply-adds: acc_lo = sum x_lo[i] C[i] + (k mod 2^58), acc_hi = sum x_hi[i] C[i] + ((k >> 58) << 26)
// -- together k + sum x[i] C[i] in fold96's lo + hi 2^32 form.  Every coefficient of the circulant is an inline constant (<= 41; row 0's own
// element: 17 + MDS_MATRIX_DIAG[0] = 25), so the coefficients need no registers at all, and the round constant rides in as the 64-bit addend
// of the first multiply-add of each half (split by the scalar unit: no VALU) -- before round 5 it cost a multiply-add by 1 per half (the
// compiler would not take it as an addend: zero-extended SGPR pairs for 24 halves spilled, and a chain started in inline asm is re-associated
// into a separate sum + a 64-bit add).  x: the row's twelve inputs in circulant order (x[0] = the row's own element).
// Bounds for fold96: acc_lo < 2^58 + 2^41, acc_hi < 2^32 + 2^41: T = hi_hi (2^32 - 1) + acc_lo stays far below 2^64.
#define POSEIDON_ROW_OPERANDS                                                                                                              \
    "v"(xl[0]), "v"(xl[1]), "v"(xl[2]), "v"(xl[3]), "v"(xl[4]), "v"(xl[5]), "v"(xl[6]), "v"(xl[7]), "v"(xl[8]), "v"(xl[9]), "v"(xl[10]),   \
    "v"(xl[11]), "v"(xh[0]), "v"(xh[1]), "v"(xh[2]), "v"(xh[3]), "v"(xh[4]), "v"(xh[5]), "v"(xh[6]), "v"(xh[7]), "v"(xh[8]), "v"(xh[9]),  \
    "v"(xh[10]), "v"(xh[11])
template <bool ROW0, bool WITH_K>
__device__ __forceinline__ void mds_row(const u32* xl, const u32* xh, u64 k, u64& acc_lo, u64& acc_hi) {
    if constexpr (WITH_K) {
        if constexpr (ROW0)
            asm("s_mov_b32 s82, %26\n\t"
            "s_and_b32 s83, %27, 0x03ffffff\n\t"
            "s_and_b32 s84, %27, 0xfc000000\n\t"
            "s_mov_b32 s85, 0\n\t"
            "v_mad_u64_u32 %0, vcc, %2, 25, s[82:83]\n\t"
            "v_mad_u64_u32 %1, vcc, %14, 25, s[84:85]\n\t"
            "v_mad_u64_u32 %0, vcc, %3, 15, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %15, 15, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %4, 41, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %16, 41, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %5, 16, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %17, 16, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %6, 2, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %18, 2, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %7, 28, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %19, 28, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %8, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %20, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %9, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %21, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %10, 39, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %22, 39, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %11, 18, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %23, 18, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %12, 34, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %24, 34, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %13, 20, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %25, 20, %1"
                : "=&v"(acc_lo), "=&v"(acc_hi)
                : POSEIDON_ROW_OPERANDS, "s"((u32)k), "s"((u32)(k >> 32))
                : "vcc", "scc", "s82", "s83", "s84", "s85");
        else
            asm("s_mov_b32 s82, %26\n\t"
            "s_and_b32 s83, %27, 0x03ffffff\n\t"
            "s_and_b32 s84, %27, 0xfc000000\n\t"
            "s_mov_b32 s85, 0\n\t"
            "v_mad_u64_u32 %0, vcc, %2, 17, s[82:83]\n\t"
            "v_mad_u64_u32 %1, vcc, %14, 17, s[84:85]\n\t"
            "v_mad_u64_u32 %0, vcc, %3, 15, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %15, 15, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %4, 41, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %16, 41, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %5, 16, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %17, 16, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %6, 2, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %18, 2, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %7, 28, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %19, 28, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %8, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %20, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %9, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %21, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %10, 39, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %22, 39, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %11, 18, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %23, 18, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %12, 34, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %24, 34, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %13, 20, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %25, 20, %1"
                : "=&v"(acc_lo), "=&v"(acc_hi)
                : POSEIDON_ROW_OPERANDS, "s"((u32)k), "s"((u32)(k >> 32))
                : "vcc", "scc", "s82", "s83", "s84", "s85");
    } else {
        if constexpr (ROW0)
            asm("v_mad_u64_u32 %0, vcc, %2, 25, 0\n\t"
            "v_mad_u64_u32 %1, vcc, %14, 25, 0\n\t"
            "v_mad_u64_u32 %0, vcc, %3, 15, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %15, 15, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %4, 41, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %16, 41, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %5, 16, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %17, 16, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %6, 2, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %18, 2, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %7, 28, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %19, 28, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %8, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %20, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %9, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %21, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %10, 39, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %22, 39, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %11, 18, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %23, 18, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %12, 34, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %24, 34, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %13, 20, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %25, 20, %1"
                : "=&v"(acc_lo), "=&v"(acc_hi)
                : POSEIDON_ROW_OPERANDS
                : "vcc");
        else
            asm("v_mad_u64_u32 %0, vcc, %2, 17, 0\n\t"
            "v_mad_u64_u32 %1, vcc, %14, 17, 0\n\t"
            "v_mad_u64_u32 %0, vcc, %3, 15, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %15, 15, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %4, 41, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %16, 41, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %5, 16, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %17, 16, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %6, 2, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %18, 2, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %7, 28, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %19, 28, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %8, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %20, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %9, 13, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %21, 13, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %10, 39, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %22, 39, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %11, 18, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %23, 18, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %12, 34, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %24, 34, %1\n\t"
            "v_mad_u64_u32 %0, vcc, %13, 20, %0\n\t"
            "v_mad_u64_u32 %1, vcc, %25, 20, %1"
                : "=&v"(acc_lo), "=&v"(acc_hi)
                : POSEIDON_ROW_OPERANDS
                : "vcc");
    }
}
#endif

// s <- MDS * s + k (kc: the 12 constants, already in registers; nullptr: none).  s: any u64 residues.
GL_HD void mds_add_const(u64* s, const u64* kc) {
    u32 lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        lo[i] = (u32)s[i];
        hi[i] = (u32)(s[i] >> 32);
    }
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        u64 acc_lo, acc_hi;
#if defined(__HIP_DEVICE_COMPILE__)
        u32 xl[12], xh[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            xl[i] = lo[(i + r) % 12];
            xh[i] = hi[(i + r) % 12];
        }
        if (kc) {
            if (r == 0) mds_row<true, true>(xl, xh, kc[r], acc_lo, acc_hi);
            else mds_row<false, true>(xl, xh, kc[r], acc_lo, acc_hi);
        } else {
            if (r == 0) mds_row<true, false>(xl, xh, 0, acc_lo, acc_hi);
            else mds_row<false, false>(xl, xh, 0, acc_lo, acc_hi);
        }
#else
        const u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
        const u64 k = kc ? kc[r] : 0;
        acc_lo = (u32)k, acc_hi = k >> 32;
        for (int i = 0; i < 12; ++i) {
            const u32 c = r == 0 && i == 0 ? C[0] + 8 : C[i];   // row 0: MDS_MATRIX_DIAG[0] = 8 joins the circulant's entry for the same element
            acc_lo += (u64)lo[(i + r) % 12] * c;
            acc_hi += (u64)hi[(i + r) % 12] * c;
        }
#endif
        s[r] = fold96(acc_lo, acc_hi);
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
// One row of a fused partial-round group: acc = d3 M1 + d2 m2 + sum x[j] m3[j] + k in fold96's lo + hi 2^32 form, as ONE block of 28
// multiply-adds -- the two halves interleaved, each starting with the constant's share as the 64-bit addend of its first multiply-add (M1, an
// entry of M itself, is an inline constant; the entries of M^2 and M^3 are scalar operands).  The constant is split INSIDE the block on the
// scalar unit (low half: k mod 2^58; high half: (k >> 58) << 26), into the block's own scratch pair: handed in as two ready-made 64-bit
// operands (round 5) the compiler computed all 24 of a group ahead of the S-boxes and spilled them to VGPR lanes (66 SGPR spills in
// leaf_hash_kernel, ~140 v_readlane / v_writelane per permutation: VERDICT r05 weak 3); now the raw constants stay where the scalar loads put them.
template <unsigned M1>
__device__ __forceinline__ void group_row(u32 d3l, u32 d3h, u32 d2l, u32 d2h, u32 m2, u64 k, const u32* xl, const u32* xh, const u32* m3, u64& acc_lo,
                                          u64& acc_hi) {
    static_assert(M1 <= 64, "inline constant");
    asm("s_mov_b32 s82, %43\n\t"
        "s_and_b32 s83, %44, 0x03ffffff\n\t"
        "s_and_b32 s84, %44, 0xfc000000\n\t"
        "s_mov_b32 s85, 0\n\t"
        "v_mad_u64_u32 %0, vcc, %2, %45, s[82:83]\n\t"
        "v_mad_u64_u32 %1, vcc, %3, %45, s[84:85]\n\t"
        "v_mad_u64_u32 %0, vcc, %4, %6, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %5, %6, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %7, %31, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %19, %31, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %8, %32, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %20, %32, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %9, %33, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %21, %33, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %10, %34, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %22, %34, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %11, %35, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %23, %35, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %12, %36, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %24, %36, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %13, %37, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %25, %37, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %14, %38, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %26, %38, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %15, %39, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %27, %39, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %16, %40, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %28, %40, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %17, %41, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %29, %41, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %18, %42, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %30, %42, %1"
        : "=&v"(acc_lo), "=&v"(acc_hi)
        : "v"(d3l), "v"(d3h), "v"(d2l), "v"(d2h), "s"(m2),                                                                           // 2..6
          "v"(xl[0]), "v"(xl[1]), "v"(xl[2]), "v"(xl[3]), "v"(xl[4]), "v"(xl[5]), "v"(xl[6]), "v"(xl[7]), "v"(xl[8]), "v"(xl[9]), "v"(xl[10]),
          "v"(xl[11]),                                                                                                             // 7..18
          "v"(xh[0]), "v"(xh[1]), "v"(xh[2]), "v"(xh[3]), "v"(xh[4]), "v"(xh[5]), "v"(xh[6]), "v"(xh[7]), "v"(xh[8]), "v"(xh[9]), "v"(xh[10]),
          "v"(xh[11]),                                                                                                             // 19..30
          "s"(m3[0]), "s"(m3[1]), "s"(m3[2]), "s"(m3[3]), "s"(m3[4]), "s"(m3[5]), "s"(m3[6]), "s"(m3[7]), "s"(m3[8]), "s"(m3[9]), "s"(m3[10]),
          "s"(m3[11]),                                                                                                             // 31..42
          "s"((u32)k), "s"((u32)(k >> 32)), "n"(M1)                                                                                // 43..45
        : "vcc", "scc", "s82", "s83", "s84", "s85");
}
template <int I> struct GroupRow {
    static __device__ __forceinline__ void run(u64* s, const u64* kv, const u32* lo, const u32* hi, u32 d2l, u32 d2h, u32 d3l, u32 d3h) {
        u32 m3[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) m3[j] = MDS3[I][j];
        u64 acc_lo, acc_hi;
        group_row<MDS1[I][0]>(d3l, d3h, d2l, d2h, MDS2[I][0], kv[I], lo, hi, m3, acc_lo, acc_hi);
        s[I] = fold96(acc_lo, acc_hi);
        if constexpr (I + 1 < 12) GroupRow<I + 1>::run(s, kv, lo, hi, d2l, d2h, d3l, d3h);
    }
};
#endif

// Three consecutive partial rounds in one dense pass (derivation and bounds: tools/gen_poseidon_partial_groups.py).
// The MDS entries are so small that M^2 and M^3 still fit 32-bit multiplicands with room in 64-bit accumulators, so
// instead of 3 x (288 multiply-adds + 12 folds) a group costs 288 (M^3) + 24 + 26 (row 0 of M, M^2) + 48 (the two
// inner S-box corrections) multiply-adds and 14 folds.  s: x1 on entry (round constants included), x1' on exit.
// GATE = true is the PoseidonGate form of the same three rounds (gates.hip): the S-box inputs are the gate's partial_sbox wires
// w[0..3) instead of the computed values, and the computed inputs of rounds 2 and 3 are returned (canonical) in x_out[0..2)
// for the constraints "computed - wire" (round 1's input is s[0] on entry).  GATE = false with x_out != nullptr is the witness
// generator's form: the plain permutation that also reports those two S-box inputs (the gate's wires).
template <bool GATE> GL_HD void partial_group3_core(u64* s, const PartialGroup& G, const u64* w, u64* x_out) {
    // request the group's constants before the first S-box (scalar-load latency hidden under it)
    const u64 k2 = G.k2, k3 = G.k3;
    u64 kv[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) kv[i] = G.kvec[i];
    s[0] = sbox(GATE ? w[0] : s[0]);
    u32 lo[12], hi[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        lo[j] = (u32)s[j];
        hi[j] = (u32)(s[j] >> 32);
    }
    // x2_0 = (M y)[0] + c2[0]
    u64 a_lo = (u32)k2, a_hi = k2 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        a_lo += (u64)lo[j] * MDS1[0][j];
        a_hi += (u64)hi[j] * MDS1[0][j];
    }
    // x2, x3 are canonical only where somebody asks for them (the gate's constraints, the generator's wires); the permutation itself runs on
    // residues: S-box, the difference d (gl::sub_a takes any residues) and its 32-bit halves as multiplicands (round 5: 16 instructions
    // per group fewer in the hashing kernels)
    u64 x2 = fold96(a_lo, a_hi);
    if (GATE || x_out) {
        x2 = gl::canon(x2);
        x_out[0] = x2;
    }
    const u64 d2 = gl::sub_a(sbox(GATE ? w[1] : x2), x2);
    const u32 d2l = (u32)d2, d2h = (u32)(d2 >> 32);
    // x3_0 = (M^2 y)[0] + M[0][0] d2 + (M c2)[0] + c3[0]
    u64 b_lo = (u32)k3, b_hi = k3 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        b_lo += (u64)lo[j] * MDS2[0][j];
        b_hi += (u64)hi[j] * MDS2[0][j];
    }
    b_lo += (u64)d2l * MDS1[0][0];
    b_hi += (u64)d2h * MDS1[0][0];
    u64 x3 = fold96(b_lo, b_hi);
    if (GATE || x_out) {
        x3 = gl::canon(x3);
        x_out[1] = x3;
    }
    const u64 d3 = gl::sub_a(sbox(GATE ? w[2] : x3), x3);
    const u32 d3l = (u32)d3, d3h = (u32)(d3 >> 32);
    // x1' = M^3 y + d2 (M^2 e0) + d3 (M e0) + kvec
#if defined(__HIP_DEVICE_COMPILE__)
    GroupRow<0>::run(s, kv, lo, hi, d2l, d2h, d3l, d3h);
#else
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const u64 k = kv[i];
        u64 acc_lo = (u32)k, acc_hi = k >> 32;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            acc_lo += (u64)lo[j] * MDS3[i][j];
            acc_hi += (u64)hi[j] * MDS3[i][j];
        }
        acc_lo += (u64)d2l * MDS2[i][0] + (u64)d3l * MDS1[i][0];
        acc_hi += (u64)d2h * MDS2[i][0] + (u64)d3h * MDS1[i][0];
        s[i] = fold96(acc_lo, acc_hi);
    }
#endif
}
template <bool GATE> GL_HD void partial_group3_core(u64* s, int g, const u64* w, u64* x_out) {
    partial_group3_core<GATE>(s, partial_group(g), w, x_out);
}
GL_HD void partial_group3(u64* s, int g) { partial_group3_core<false>(s, g, nullptr, nullptr); }

// ---- the closing group of FOUR partial rounds (rounds 22..25) of the hashing permutation ----
// In place of the seventh group of three and the lone round 25 (a whole MDS layer for one S-box).  Derivation, constants and the exact bounds:
// tools/gen_poseidon_partial_groups.py.  A row of M^4 sums to more than 2^32, so one accumulator of 32-bit halves times M^4 could pass 2^64;
// but every entry of row i lies within 2^24.1 of the row's smallest, MDS4_BASE[i]: M^4 = N + b 1^T.  The sum of the twelve words is taken
// once and folded to a residue t, and row i is  N[i] . y + b_i t + d2 M^3[i][0] + d3 M^2[i][0] + d4 M[i][0] + kvec[i]  -- 32 multiply-adds per half
// pair, every accumulator below 2^61, fold96 as it is.  486 multiply-adds and 16 folds against the 674 and 26 of a group of three + round 25.
static const ClosingGroup CG_HOST = POSEIDON_CLOSING_GROUP_INIT;
#if defined(__HIPCC__)
static __constant__ ClosingGroup CG_DEV = POSEIDON_CLOSING_GROUP_INIT;
#endif
// z: a zero (permute_head's opaque one: the constants are then loaded where they are used, not once in front of a sponge loop)
GL_HD const ClosingGroup& closing_group(int z) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (&CG_DEV)[z];
#else
    return (&CG_HOST)[z];
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
// sum_lo = the sum of the twelve low halves, sum_hi = of the twelve high halves (each < 12 * 2^32): 24 multiply-adds by the inline constant 1
__device__ __forceinline__ void halves_sum(const u32* xl, const u32* xh, u64& sum_lo, u64& sum_hi) {
    asm("v_mad_u64_u32 %0, vcc, %2, 1, 0\n\t"
        "v_mad_u64_u32 %1, vcc, %14, 1, 0\n\t"
        "v_mad_u64_u32 %0, vcc, %3, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %15, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %4, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %16, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %5, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %17, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %6, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %18, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %7, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %19, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %8, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %20, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %9, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %21, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %10, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %22, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %11, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %23, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %12, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %24, 1, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %13, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %25, 1, %1"
        : "=&v"(sum_lo), "=&v"(sum_hi)
        : POSEIDON_ROW_OPERANDS
        : "vcc");
}
// One row of the closing group as ONE block of 32 multiply-adds, in the manner of group_row: the constant is split inside the block, M1 (an
// entry of M) is an inline constant, the entries of M^2, M^3, N and b are scalar operands.
template <unsigned M1>
__device__ __forceinline__ void closing_row(u32 d4l, u32 d4h, u32 d3l, u32 d3h, u32 m2, u32 d2l, u32 d2h, u32 m3, u32 tl, u32 th, u32 base, u64 k,
                                            const u32* xl, const u32* xh, const u32* n, u64& acc_lo, u64& acc_hi) {
    static_assert(M1 <= 64, "inline constant");
    asm("s_mov_b32 s82, %49\n\t"
        "s_and_b32 s83, %50, 0x03ffffff\n\t"
        "s_and_b32 s84, %50, 0xfc000000\n\t"
        "s_mov_b32 s85, 0\n\t"
        "v_mad_u64_u32 %0, vcc, %2, %51, s[82:83]\n\t"
        "v_mad_u64_u32 %1, vcc, %3, %51, s[84:85]\n\t"
        "v_mad_u64_u32 %0, vcc, %4, %6, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %5, %6, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %7, %9, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %8, %9, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %10, %12, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %11, %12, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %13, %37, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %25, %37, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %14, %38, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %26, %38, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %15, %39, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %27, %39, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %16, %40, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %28, %40, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %17, %41, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %29, %41, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %18, %42, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %30, %42, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %19, %43, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %31, %43, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %20, %44, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %32, %44, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %21, %45, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %33, %45, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %22, %46, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %34, %46, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %23, %47, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %35, %47, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %24, %48, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %36, %48, %1"
        : "=&v"(acc_lo), "=&v"(acc_hi)
        : "v"(d4l), "v"(d4h),                                                                                                      // 2..3
          "v"(d3l), "v"(d3h), "s"(m2), "v"(d2l), "v"(d2h), "s"(m3), "v"(tl), "v"(th), "s"(base),                                     // 4..12
          "v"(xl[0]), "v"(xl[1]), "v"(xl[2]), "v"(xl[3]), "v"(xl[4]), "v"(xl[5]), "v"(xl[6]), "v"(xl[7]), "v"(xl[8]), "v"(xl[9]), "v"(xl[10]),
          "v"(xl[11]),                                                                                                             // 13..24
          "v"(xh[0]), "v"(xh[1]), "v"(xh[2]), "v"(xh[3]), "v"(xh[4]), "v"(xh[5]), "v"(xh[6]), "v"(xh[7]), "v"(xh[8]), "v"(xh[9]), "v"(xh[10]),
          "v"(xh[11]),                                                                                                             // 25..36
          "s"(n[0]), "s"(n[1]), "s"(n[2]), "s"(n[3]), "s"(n[4]), "s"(n[5]), "s"(n[6]), "s"(n[7]), "s"(n[8]), "s"(n[9]), "s"(n[10]),
          "s"(n[11]),                                                                                                              // 37..48
          "s"((u32)k), "s"((u32)(k >> 32)), "n"(M1)                                                                                // 49..51
        : "vcc", "scc", "s82", "s83", "s84", "s85");
}
template <int I> struct ClosingRow {
    static __device__ __forceinline__ void run(u64* s, const u64* kv, const u32* lo, const u32* hi, u32 d2l, u32 d2h, u32 d3l, u32 d3h, u32 d4l, u32 d4h,
                                               u32 tl, u32 th) {
        u32 n[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) n[j] = MDS4[I][j] - MDS4_BASE[I];
        u64 acc_lo, acc_hi;
        closing_row<MDS1[I][0]>(d4l, d4h, d3l, d3h, MDS2[I][0], d2l, d2h, MDS3[I][0], tl, th, MDS4_BASE[I], kv[I], lo, hi, n, acc_lo, acc_hi);
        s[I] = fold96(acc_lo, acc_hi);
        if constexpr (I + 1 < 12) ClosingRow<I + 1>::run(s, kv, lo, hi, d2l, d2h, d3l, d3h, d4l, d4h, tl, th);
    }
};
#endif
// s: round 22's input (its constants included) on entry, round 26's on exit; any residues in, residues out.  WIRES = true is the form the layer
// tests steer: the four S-box inputs are w[0..4) instead of the computed values (as the gate form of partial_group3_core does it), which lets a
// test place d2, d3, d4 where the accumulators peak; the permutation runs WIRES = false.
template <bool WIRES> GL_HD void closing_group4_core(u64* s, const ClosingGroup& G, const u64* w) {
    const u64 k2 = G.k2, k3 = G.k3, k4 = G.k4;
    u64 kv[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) kv[i] = G.kvec[i];
    s[0] = sbox(WIRES ? w[0] : s[0]);
    u32 lo[12], hi[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        lo[j] = (u32)s[j];
        hi[j] = (u32)(s[j] >> 32);
    }
    // x2_0 = (M y)[0] + c2[0]
    u64 a_lo = (u32)k2, a_hi = k2 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        a_lo += (u64)lo[j] * MDS1[0][j];
        a_hi += (u64)hi[j] * MDS1[0][j];
    }
    const u64 x2 = fold96(a_lo, a_hi);
    const u64 d2 = gl::sub_a(sbox(WIRES ? w[1] : x2), x2);
    const u32 d2l = (u32)d2, d2h = (u32)(d2 >> 32);
    // x3_0 = (M^2 y)[0] + M[0][0] d2 + k3
    u64 b_lo = (u32)k3, b_hi = k3 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        b_lo += (u64)lo[j] * MDS2[0][j];
        b_hi += (u64)hi[j] * MDS2[0][j];
    }
    b_lo += (u64)d2l * MDS1[0][0];
    b_hi += (u64)d2h * MDS1[0][0];
    const u64 x3 = fold96(b_lo, b_hi);
    const u64 d3 = gl::sub_a(sbox(WIRES ? w[2] : x3), x3);
    const u32 d3l = (u32)d3, d3h = (u32)(d3 >> 32);
    // x4_0 = (M^3 y)[0] + M^2[0][0] d2 + M[0][0] d3 + k4
    u64 c_lo = (u32)k4, c_hi = k4 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        c_lo += (u64)lo[j] * MDS3[0][j];
        c_hi += (u64)hi[j] * MDS3[0][j];
    }
    c_lo += (u64)d2l * MDS2[0][0] + (u64)d3l * MDS1[0][0];
    c_hi += (u64)d2h * MDS2[0][0] + (u64)d3h * MDS1[0][0];
    const u64 x4 = fold96(c_lo, c_hi);
    const u64 d4 = gl::sub_a(sbox(WIRES ? w[3] : x4), x4);
    const u32 d4l = (u32)d4, d4h = (u32)(d4 >> 32);
    // t = the sum of the twelve words as one residue: the share of M^4 that every row has in common
    u64 t_lo, t_hi;
#if defined(__HIP_DEVICE_COMPILE__)
    halves_sum(lo, hi, t_lo, t_hi);
#else
    t_lo = 0, t_hi = 0;
    for (int j = 0; j < 12; ++j) {
        t_lo += lo[j];
        t_hi += hi[j];
    }
#endif
    const u64 t = fold96(t_lo, t_hi);
    const u32 tl = (u32)t, th = (u32)(t >> 32);
    // x1' = N y + b t + d2 (M^3 e0) + d3 (M^2 e0) + d4 (M e0) + kvec
#if defined(__HIP_DEVICE_COMPILE__)
    ClosingRow<0>::run(s, kv, lo, hi, d2l, d2h, d3l, d3h, d4l, d4h, tl, th);
#else
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const u64 k = kv[i];
        u64 acc_lo = (u32)k, acc_hi = k >> 32;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            acc_lo += (u64)lo[j] * (MDS4[i][j] - MDS4_BASE[i]);
            acc_hi += (u64)hi[j] * (MDS4[i][j] - MDS4_BASE[i]);
        }
        acc_lo += (u64)tl * MDS4_BASE[i] + (u64)d2l * MDS3[i][0] + (u64)d3l * MDS2[i][0] + (u64)d4l * MDS1[i][0];
        acc_hi += (u64)th * MDS4_BASE[i] + (u64)d2h * MDS3[i][0] + (u64)d3h * MDS2[i][0] + (u64)d4h * MDS1[i][0];
        s[i] = fold96(acc_lo, acc_hi);
    }
#endif
}
GL_HD void closing_group4(u64* s, int z = 0) { closing_group4_core<false>(s, closing_group(z), nullptr); }

// The permutation up to and including the S-boxes of the last round: everything but the last MDS layer, which adds no constants and of which a
// sponge reads a few rows only (last_rows below).  in: any u64 residues; out: the twelve S-box outputs of round 29 (residues).
GL_HD void permute_head(u64* s) {
#if defined(__HIP_DEVICE_COMPILE__)
    // A zero the compiler cannot see through, made anew by every call: the constants of the first round and of the closing group have fixed addresses,
    // so in a sponge loop they are loop-invariant -- the compiler loaded all 48 words once, in front of the loop, found no scalar registers to
    // keep them in and parked them in VGPR lanes: 48 v_readlane per permutation, where a scalar load costs the vector
    // unit nothing.  Indexed by this zero they are loaded where they are used.
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
#else
    constexpr int z = 0;
#endif
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = gl::add_nc(s[i], rc(z + i));
    // the next round's constants are requested (scalar loads) BEFORE the S-boxes so their latency hides under ~800
    // instructions instead of parking the wave right in front of the MDS layer (17 % of wave cycles in the first version)
    for (int r = 0; r < HALF_FULL; ++r) {
        u64 kc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) kc[i] = rc(12 * (r + 1) + i);
#pragma unroll
        for (int i = 0; i < 12; i += 2) sbox2(s[i], s[i + 1]);
        mds_add_const(s, kc);
    }
    // 22 partial rounds = 6 fused groups of 3 (rounds 4..21) + the closing group of 4 (rounds 22..25).  (The seventh group of three and the plain
    // round 25 that the gate and the witness generators run give the same values: tools/gen_poseidon_partial_groups.py checks both.)
    {
        // (the table's address is re-derived by the compiler in front of every group -- one scalar load from the constant pool; making the
        // pointer opaque to stop that turns the group's constants into vector loads: measured, worse)
        for (int g = 0; g < 6; ++g) partial_group3(s, g);
    }
    {
#if defined(__HIP_DEVICE_COMPILE__)
        int z4;   // a zero of its own: the first one would have to live through 10 k instructions
        asm volatile("s_mov_b32 %0, 0" : "=s"(z4));
#else
        constexpr int z4 = 0;
#endif
        closing_group4(s, z4);
    }
    for (int r = HALF_FULL + N_PARTIAL; r < N_ROUNDS - 1; ++r) {
        u64 kc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) kc[i] = rc(12 * (r + 1) + i);
#pragma unroll
        for (int i = 0; i < 12; i += 2) sbox2(s[i], s[i + 1]);
        mds_add_const(s, kc);
    }
#pragma unroll
    for (int i = 0; i < 12; i += 2) sbox2(s[i], s[i + 1]);
}
// The 32-bit halves of permute_head's result: what every row of the last layer reads.  Taken once, so that rows written into s do not disturb
// the rows computed after them.
struct HeadHalves {
    u32 lo[12], hi[12];
};
GL_HD HeadHalves head_halves(const u64* s) {
    HeadHalves h;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        h.lo[i] = (u32)s[i];
        h.hi[i] = (u32)(s[i] >> 32);
    }
    return h;
}
// Rows FIRST .. FIRST + COUNT of the last MDS layer (no constants): s[r] <- (M y)[r] for those r, y = the head's result in halves.  The other
// elements of s are NOT written: they keep the head's S-box outputs, which are no part of the permutation's result -- nobody may read them.
template <int FIRST, int COUNT> GL_HD void last_rows(u64* s, const HeadHalves& h) {
    static_assert(FIRST >= 0 && COUNT > 0 && FIRST + COUNT <= 12, "rows of a width-12 state");
#pragma unroll
    for (int r = FIRST; r < FIRST + COUNT; ++r) {
        u64 acc_lo, acc_hi;
#if defined(__HIP_DEVICE_COMPILE__)
        u32 xl[12], xh[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            xl[i] = h.lo[(i + r) % 12];
            xh[i] = h.hi[(i + r) % 12];
        }
        if (r == 0) mds_row<true, false>(xl, xh, 0, acc_lo, acc_hi);
        else mds_row<false, false>(xl, xh, 0, acc_lo, acc_hi);
#else
        const u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
        acc_lo = 0, acc_hi = 0;
        for (int i = 0; i < 12; ++i) {
            const u32 c = r == 0 && i == 0 ? C[0] + 8 : C[i];
            acc_lo += (u64)h.lo[(i + r) % 12] * c;
            acc_hi += (u64)h.hi[(i + r) % 12] * c;
        }
#endif
        s[r] = fold96(acc_lo, acc_hi);
    }
}

// in: any u64 residues; out: u64 residues (the caller makes canonical what leaves the sponge -- a chain of absorbs needs that for the digest
// only: 48 instructions per permutation otherwise)
GL_HD void permute_residues(u64* s) {
    permute_head(s);
    last_rows<0, 12>(s, head_halves(s));
}
// The permutation of an overwrite-mode sponge of rate 8 (hash/hashing.rs `hash_n_to_m_no_pad`) together with the absorb that follows it.  Such a
// sponge reads only part of the permutation's result, and only those rows of the last MDS layer are computed (a row is 24 multiply-adds and a fold):
//   last block            -> the digest s[0..4): rows 0..3.  s[4..12) are NOT the permutation's.
//   a full block follows  -> it replaces s[0..8): rows 8..11, the capacity, then absorb(8).
//   a partial one follows -> it replaces s[0..n), n < 8: all twelve rows, then absorb(n).
// absorb(n) writes the next block's n words over s[0..n) (n = 8: a full block); it runs in here, on the branch that knows which rows exist, so
// that nothing can read an element the layer left out.  remaining: the words the sponge has yet to absorb, this permutation's block included
// (<= 8: the last block; < 16: a partial block follows); it must be wave-uniform (scalar branches).  Returns whether a block was absorbed, that
// is whether the sponge goes on.  The head exists ONCE.
template <class Absorb> GL_HD bool permute_sponge(u64* s, unsigned remaining, Absorb&& absorb) {
    permute_head(s);
#if defined(__HIP_DEVICE_COMPILE__)
    // every decision is taken HERE, from the one count, the caller's loop condition included: made in front of the head (where they are the
    // comparisons that guard the prefetch) they would be carried through its 12 k instructions as lane masks -- scalar pairs, which a sponge
    // kernel can only park in VGPR lanes
    asm volatile("" : "+s"(remaining));
#endif
    const HeadHalves h = head_halves(s);
    if (remaining <= 8) {
        last_rows<0, 4>(s, h);
        return false;
    }
    last_rows<8, 4>(s, h);
    if (remaining < 16) {
        last_rows<0, 8>(s, h);
        absorb(remaining - 8);
    } else {
        absorb(8u);
    }
    return true;
}
// a sponge's only or last permutation: the digest s[0..4)
GL_HD void permute_digest(u64* s) {
    permute_head(s);
    last_rows<0, 4>(s, head_halves(s));
}
// in: any residues (canonical inputs included); out: canonical field elements
GL_HD void permute(u64* s) {
    permute_residues(s);
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = gl::canon(s[i]);
}

#if defined(__HIPCC__)
// Latency-oriented form: one permutation spread over 16 lanes (lane l < 12 owns state element l; lanes 12..15 idle).
// Used where there are too few independent permutations to fill the chip (upper Merkle levels, FRI trees): the
// lane-per-permutation form has a ~65 us dependent-instruction chain; here the 12 S-boxes of a full round and the 12
// MDS rows run side by side and the state is exchanged through LDS (one ds_write_b64 + 12 ds_read_b64 per round).
// `sh` points at this 16-lane group's private 24-word LDS window (element l is stored at l and l + 12 so the
// circulant index needs no modulo).  All 64 lanes of the wave must call it together.  Returns the canonical value.
constexpr int WIDE_LANES = 16, WIDE_LDS_WORDS = 48;  // 48-word stride keeps the four groups of a wave on disjoint banks
__device__ __forceinline__ u64 permute_wide(u64 x, u64* sh, unsigned l) {
    constexpr u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    const unsigned row = l < 12 ? l : 0;
    // this lane's row of M^3 and its entries of the first columns of M^2 and M (fused partial rounds below)
    u32 m3[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) m3[j] = MDS3[row][j];
    const u32 m2c = MDS2[row][0], m1c = MDS1[row][0];
    x = gl::add_nc(x, rc(row));
    // this lane's round constants are fetched up front (16 independent loads, one memory latency) instead of one exposed
    // lane-indexed load per round on the dependent chain
    u64 kplain[9], kgroup[7];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int r = i < 4 ? i : HALF_FULL + N_PARTIAL - 1 + (i - 4);  // plain rounds: 0..3, 25, 26..29
        kplain[i] = r + 1 < N_ROUNDS ? rc(12 * (r + 1) + row) : 0;
    }
#pragma unroll
    for (int g = 0; g < 7; ++g) kgroup[g] = partial_group(g).kvec[row];
    // one plain round: S-box (full: every lane; partial: lane 0), exchange through LDS, this lane's MDS row + next constants
    auto plain_round = [&](u64 k, bool full) {
        if (full || l == 0) x = sbox_ilp(x);
        // the 16 lanes of a group live in one wave: LDS operations of a wave execute in order, so a wavefront-scope
        // fence (compiler ordering only) is all the synchronisation the exchange needs
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (l < 12) {
            sh[l] = x;
            sh[l + 12] = x;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // three independent accumulator chains per half (latency: 4 dependent multiply-adds instead of 12)
        u64 al[3] = {(u32)k, 0, 0}, ah[3] = {k >> 32, 0, 0};
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const u64 v = sh[row + i];
            al[i % 3] += (u64)(u32)v * C[i];
            ah[i % 3] += (v >> 32) * C[i];
        }
        if (l == 0) {
            al[1] += (u64)(u32)x * 8u;
            ah[1] += (x >> 32) * 8u;
        }
        x = fold96(al[0] + al[1] + al[2], ah[0] + ah[1] + ah[2]);
    };
#pragma unroll
    for (int i = 0; i < HALF_FULL; ++i) plain_round(kplain[i], true);
    // 21 partial rounds as 7 fused groups of three (same algebra as partial_group3_core): ONE exchange per group.  After it every
    // lane holds the whole post-S-box state y, so every lane computes the two inner S-box inputs x2_0 = (M y)[0] + k2 and
    // x3_0 = (M^2 y)[0] + M00 d2 + k3 redundantly (no broadcast), and its own row of M^3 y + d2 M^2[:,0] + d3 M[:,0] + kvec.
    // The M^3 row and most of the x3 dot product do not depend on the inner S-boxes: independent work for the scheduler to place
    // inside their dependent chains.  Critical path per group: 3 S-boxes + 1 LDS round trip instead of 3 + 3.
#pragma unroll
    for (int g = 0; g < 7; ++g) {
        const PartialGroup& G = partial_group(g);
        const u64 k2 = G.k2, k3 = G.k3, kv = kgroup[g];
        if (l == 0) x = sbox_ilp(x);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (l < 12) sh[l] = x;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        u32 lo[12], hi[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const u64 v = sh[j];
            lo[j] = (u32)v;
            hi[j] = (u32)(v >> 32);
        }
        u64 a_lo[2] = {(u32)k2, 0}, a_hi[2] = {k2 >> 32, 0};      // x2_0
        u64 b_lo[2] = {(u32)k3, 0}, b_hi[2] = {k3 >> 32, 0};      // x3_0 without the d2 term
        u64 c_lo[3] = {(u32)kv, 0, 0}, c_hi[3] = {kv >> 32, 0, 0};  // this lane's row of M^3 y + kvec
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            a_lo[j % 2] += (u64)lo[j] * MDS1[0][j];
            a_hi[j % 2] += (u64)hi[j] * MDS1[0][j];
            b_lo[j % 2] += (u64)lo[j] * MDS2[0][j];
            b_hi[j % 2] += (u64)hi[j] * MDS2[0][j];
            c_lo[j % 3] += (u64)lo[j] * m3[j];
            c_hi[j % 3] += (u64)hi[j] * m3[j];
        }
        const u64 x2 = gl::canon(fold96(a_lo[0] + a_lo[1], a_hi[0] + a_hi[1]));
        const u64 d2 = gl::sub(gl::canon(sbox_ilp(x2)), x2);
        const u32 d2l = (u32)d2, d2h = (u32)(d2 >> 32);
        const u64 x3 = gl::canon(fold96(b_lo[0] + b_lo[1] + (u64)d2l * MDS1[0][0], b_hi[0] + b_hi[1] + (u64)d2h * MDS1[0][0]));
        const u64 d3 = gl::sub(gl::canon(sbox_ilp(x3)), x3);
        const u32 d3l = (u32)d3, d3h = (u32)(d3 >> 32);
        x = fold96(c_lo[0] + c_lo[1] + c_lo[2] + (u64)d2l * m2c + (u64)d3l * m1c, c_hi[0] + c_hi[1] + c_hi[2] + (u64)d2h * m2c + (u64)d3h * m1c);
    }
#pragma unroll
    for (int i = 4; i < 9; ++i) plain_round(kplain[i], i > 4);
    return gl::canon(x);
}
#endif

// host-side permutation (Fiat-Shamir transcript: ~125 permutations per step proof between GPU phases).  An AVX2-compiled clone of
// the same code was measured: 35 % faster on the authoring container's Xeon, 13 % SLOWER on the GPU box's EPYC 9575F (1.28 ->
// 1.45 us), so the baseline x86-64 build is what ships.
inline void permute_host(u64* s) { permute(s); }

// ---- host-side sponge helpers (hash/hashing.rs), used by the Challenger and for tiny inputs ----
inline void hash_no_pad_host(const u64* in, size_t n, u64 out[4]) {
    u64 s[12] = {0};
    for (size_t off = 0; off < n; off += 8) {
        const size_t len = n - off < 8 ? n - off : 8;
        for (size_t i = 0; i < len; ++i) s[i] = in[off + i];
        permute_host(s);
    }
    for (int i = 0; i < 4; ++i) out[i] = s[i];
}
}  // namespace poseidon

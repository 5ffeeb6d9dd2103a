// VALU issue-rate microbenchmark for gfx950, second version (round 2; answers VERDICT r01 "what's weak" #2).
//
// What differs from tools/microbench_valu.hip:
//   * every chain has its OWN source registers (no instruction reads one VGPR for two operands, no operand shared between chains);
//   * the asm statements are not `volatile` (the compiler may schedule them; each result is consumed at the end);
//   * the time is taken INSIDE the kernel, per wave, with s_memtime (shader-clock counter) and s_memrealtime (constant 100 MHz):
//     cycles per instruction need no assumed clock, and the shader clock under the load is reported;
//   * the number of waves per SIMD is controlled exactly (1, 2, 4, 8): one workgroup per CU pinned by its LDS request, 256 * w threads
//     (w <= 4) or two 1024-thread workgroups (w = 8); a workgroup's waves go round-robin over the CU's four SIMDs.
// Reported: cycles of one SIMD per wave64 instruction = (cycles one wave needed) / (instructions of one wave * waves on its SIMD).
// Build: hipcc --offload-arch=gfx950 -O3 tools/microbench_valu2.hip -o tools/microbench_valu2
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <array>
#include <map>
#include <vector>

#define CHECK(x) do { hipError_t err_ = (x); if (err_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(err_), __LINE__); return 1; } } while (0)

constexpr int ITERS = 2048;
constexpr int CHAINS = 8;      // independent dependency chains per lane
constexpr int REPS = 4;        // each chain advanced REPS times per loop iteration -> CHAINS * REPS instructions per iteration

struct Stamp {
    uint64_t c0, c1, r0, r1;
    uint32_t hw_id, xcc_id;   // HW_REG_HW_ID (wave slot, SIMD, CU, SH, SE) and HW_REG_XCC_ID: which SIMD of the chip ran the wave
};

extern __shared__ uint32_t lds_pin[];

#define PROLOGUE \
    uint32_t a[CHAINS], b[CHAINS], c[CHAINS], d[CHAINS]; \
    uint64_t q[CHAINS], q2[CHAINS], q3[CHAINS]; \
    for (int i = 0; i < CHAINS; ++i) { \
        a[i] = seed * (2 * i + 3) + threadIdx.x; b[i] = seed * (2 * i + 5) + 7 * threadIdx.x + 1; c[i] = (seed ^ (0x9E3779B9u * (i + 1))) + threadIdx.x; d[i] = c[i] * 3 + b[i]; \
        q[i] = ((uint64_t)a[i] << 32) | b[i]; q2[i] = ((uint64_t)b[i] << 32) | c[i]; q3[i] = ((uint64_t)c[i] << 32) | a[i]; \
    } \
    if (seed == 0xFFFFFFFFu) lds_pin[threadIdx.x] = seed; \
    __syncthreads(); \
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime(); \
    for (int it = 0; it < ITERS; ++it) {
#define EPILOGUE \
    } \
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime(); \
    uint32_t acc = 0; \
    for (int i = 0; i < CHAINS; ++i) acc ^= a[i] ^ b[i] ^ c[i] ^ d[i] ^ (uint32_t)q[i] ^ (uint32_t)(q[i] >> 32) ^ (uint32_t)q2[i] ^ (uint32_t)q3[i]; \
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc; \
    if ((threadIdx.x & 63) == 0) stamps[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = Stamp{c0, c1, r0, r1, __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)), __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11))};

#define EACH(...) _Pragma("unroll") for (int r = 0; r < REPS; ++r) { _Pragma("unroll") for (int i = 0; i < CHAINS; ++i) { __VA_ARGS__; } }

#define KERNEL(name, ...) \
    __global__ void __launch_bounds__(1024) name(uint32_t* out, Stamp* stamps, uint32_t seed) { PROLOGUE EACH(__VA_ARGS__) EPILOGUE }

// a = b * c + a   (three distinct VGPRs per chain)
KERNEL(k_fma_f32, asm("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(b[i]), "v"(c[i])))
// packed fp32: 2 FMAs per lane per instruction on register pairs
KERNEL(k_pk_fma_f32, asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(q[i]) : "v"(q2[i]), "v"(q3[i])))
KERNEL(k_fma_f64, asm("v_fma_f64 %0, %0, %0, %0" : "+v"(q[i])))
KERNEL(k_add_u32, asm("v_add_u32 %0, %1, %0" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_xor_b32, asm("v_xor_b32 %0, %1, %0" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_and_or_b32, asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(b[i]), "v"(c[i])))
KERNEL(k_add3_u32, asm("v_add3_u32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(b[i]), "v"(c[i])))
KERNEL(k_mul_lo_u32, asm("v_mul_lo_u32 %0, %1, %0" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_mul_hi_u32, asm("v_mul_hi_u32 %0, %1, %0" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_mad_u32_u24, asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(a[i]) : "v"(b[i]), "v"(c[i])))
// carry-writing instructions: chain i sends its carry-out to its own SGPR pair s[20+2i:21+2i], so that no two neighbouring instructions
// write the same SGPR (hipcc separates such a pair with an `s_nop 0`, which costs an issue slot and would be measured along)
#define SP(i, M) M(0, "s[40:41]", "s40", "s41", "s[56:57]", "s56", "s57") M(1, "s[42:43]", "s42", "s43", "s[58:59]", "s58", "s59") M(2, "s[44:45]", "s44", "s45", "s[60:61]", "s60", "s61") M(3, "s[46:47]", "s46", "s47", "s[62:63]", "s62", "s63") M(4, "s[48:49]", "s48", "s49", "s[64:65]", "s64", "s65") M(5, "s[50:51]", "s50", "s51", "s[66:67]", "s66", "s67") M(6, "s[52:53]", "s52", "s53", "s[68:69]", "s68", "s69") M(7, "s[54:55]", "s54", "s55", "s[70:71]", "s70", "s71")
#define KERNEL8(name, M) \
    __global__ void __launch_bounds__(1024) name(uint32_t* out, Stamp* stamps, uint32_t seed) { \
        PROLOGUE _Pragma("unroll") for (int r = 0; r < REPS; ++r) { SP(0, M) } EPILOGUE }
#define M_MAD(i, S, S0, S1, T, T0, T1) asm("v_mad_u64_u32 %0, " S ", %1, %2, %0" : "+v"(q[i]) : "v"(b[i]), "v"(c[i]) : S0, S1);
#define M_MAD_S(i, S, S0, S1, T, T0, T1) asm("v_mad_u64_u32 %0, " S ", %1, %2, %0" : "+v"(q[i]) : "v"(b[i]), "s"(seed) : S0, S1);
#define M_ADDCO(i, S, S0, S1, T, T0, T1) asm("v_add_co_u32_e64 %0, " S ", %1, %0" : "+v"(a[i]) : "v"(b[i]) : S0, S1);
#define M_ADD64(i, S, S0, S1, T, T0, T1) asm("v_add_co_u32_e64 %0, " S ", %2, %0\n\tv_addc_co_u32_e64 %1, " S ", %3, %1, " S : "+v"(a[i]), "+v"(c[i]) : "v"(b[i]), "v"(d[i]) : S0, S1);
#define M_MIX(i, S, S0, S1, T, T0, T1) M_MAD(i, S, S0, S1, T, T0, T1) asm("v_add_co_u32_e64 %0, " T ", %1, %0" : "+v"(a[i]) : "v"(d[i]) : T0, T1);
KERNEL8(k_mad_u64_u32, M_MAD)
// the same with a scalar multiplier (the MDS layer's form: coefficient in an SGPR)
KERNEL8(k_mad_u64_u32_s, M_MAD_S)
KERNEL8(k_add_co_u32, M_ADDCO)
// 64-bit add = v_add_co_u32 + v_addc_co_u32 (2 instructions, counted as 2)
KERNEL8(k_add_u64, M_ADD64)
// the mix of the Poseidon MDS / modular-multiply code: half v_mad_u64_u32, half carry adds
KERNEL8(k_mix_poseidon, M_MIX)
KERNEL(k_lshl_add_u64, asm("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(q[i]) : "v"(q[(i + 3) % CHAINS])))
KERNEL(k_cndmask, { asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b[i]), "s"((uint64_t)seed * 0x9E3779B97F4A7C15ull)); })
KERNEL(k_lshlrev_b64, asm("v_lshlrev_b64 %0, 1, %0" : "+v"(q[i])))
KERNEL(k_alignbit, asm("v_alignbit_b32 %0, %1, %0, 7" : "+v"(a[i]) : "v"(b[i])))
// ---- the rows that price a Goldilocks product in cycles: moves, the vcc-selected cndmask, the 64-bit shift that makes {hi, 0} in one
// instruction, a one-in-three mix of full-rate and half-rate instructions, and the two whole assemblies of the 128-bit product
KERNEL(k_mov_b32, asm("v_mov_b32 %0, %1" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_add_u32_mov, asm("v_add_u32 %0, 0, %1" : "+v"(a[i]) : "v"(b[i])))
// vcc as the selector: its value does not matter for the rate, the statements only have to keep their order (volatile)
KERNEL(k_cndmask_e32, asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(a[i]) : "v"(b[i])))
KERNEL(k_cndmask_e32_const, asm volatile("v_cndmask_b32_e32 %0, 0, %1, vcc" : "+v"(a[i]) : "v"(b[i])))
// the carry adds as the product forms write them: the 32-bit encodings with vcc (the rows above are the 64-bit encodings with an SGPR pair)
KERNEL(k_add_co_e32, asm volatile("v_add_co_u32_e32 %0, vcc, %1, %0" : "+v"(a[i]) : "v"(b[i]) : "vcc"))
KERNEL(k_addc_co_e32, asm volatile("v_addc_co_u32_e32 %0, vcc, %1, %0, vcc" : "+v"(a[i]) : "v"(b[i]) : "vcc"))
KERNEL(k_lshrrev_b64_32, asm("v_lshrrev_b64 %0, 32, %0" : "+v"(q[i])))
// one v_add_u32 per two v_mad_u64_u32, every chain on its own registers and its own carry SGPR pairs (the add steps a multiplicand of its
// chain: a fourth register array would put the kernel over the 64 VGPRs that 8 waves per SIMD leave)
#define M_MIX3(i, S, S0, S1, T, T0, T1) M_MAD(i, S, S0, S1, T, T0, T1) asm("v_mad_u64_u32 %0, " T ", %1, %2, %0" : "+v"(q2[i]) : "v"(c[i]), "v"(b[i]) : T0, T1); asm("v_add_u32 %0, %1, %0" : "+v"(c[i]) : "v"(b[i]));
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) k_mix_mad2_add(uint32_t* out, Stamp* stamps, uint32_t seed) {
    PROLOGUE _Pragma("unroll") for (int r = 0; r < REPS; ++r) { SP(0, M_MIX3) } EPILOGUE }
// The assembly of a0 a1 x b0 b1 -> 128 bits as in csrc/gl.h, one dependent chain per wave: a block's four result words are the next block's
// operands, the blocks alternate between two scratch sets (v40.. / v48..), so that nothing but the assembly itself is issued.  32 blocks
// per loop iteration (+ 4 moves that hand the last result to the next iteration, the same for every form: 1.5 % of the old form).
// X = a0, a1, b0, b1 of the block; R0..R7 its scratch set (P01 / P23 / P45 the aligned pairs); SG its carry SGPR pair.
#define ASM_OLD(...) ASM_OLD_(__VA_ARGS__)
#define ASM_OLD_(a0, a1, b0, b1, R0, R1, R2, R3, R4, R5, R6, P01, P23, P45, SG) \
    "v_mad_u64_u32 " P01 ", vcc, " a0 ", " b0 ", 0\n\t" \
    "v_mad_u64_u32 " P23 ", vcc, " a0 ", " b1 ", 0\n\t" \
    "v_mad_u64_u32 " P23 ", " SG ", " a1 ", " b0 ", " P23 "\n\t" \
    "v_mad_u64_u32 " P45 ", vcc, " a1 ", " b1 ", 0\n\t" \
    "v_cndmask_b32_e64 " R6 ", 0, 1, " SG "\n\t" \
    "v_add_co_u32_e32 " R1 ", vcc, " R1 ", " R2 "\n\t" \
    "v_addc_co_u32_e32 " R4 ", vcc, " R4 ", " R3 ", vcc\n\t" \
    "v_addc_co_u32_e32 " R5 ", vcc, " R5 ", " R6 ", vcc\n\t"
// chained: P = a0 b0; E = {P.hi, 0}; M = a0 b1 + E; M = a1 b0 + M (carry c); F = {M.hi, c}; H = a1 b1 + F; lo = {P.lo, M.lo}
#define ASM_CHAIN(...) ASM_CHAIN_(__VA_ARGS__)
#define ASM_CHAIN_(MOVE, ZERO_E, a0, a1, b0, b1, R0, R1, R2, R3, R4, R5, R6, P01, P23, P45, SG) \
    "v_mad_u64_u32 " P01 ", vcc, " a0 ", " b0 ", 0\n\t" \
    ZERO_E(MOVE, R1, R2, R3, P01, P23) \
    "v_mad_u64_u32 " P23 ", vcc, " a0 ", " b1 ", " P23 "\n\t" \
    "v_mad_u64_u32 " P23 ", " SG ", " a1 ", " b0 ", " P23 "\n\t" \
    MOVE(R4, R3) \
    "v_cndmask_b32_e64 " R5 ", 0, 1, " SG "\n\t" \
    "v_mad_u64_u32 " P45 ", vcc, " a1 ", " b1 ", " P45 "\n\t" \
    MOVE(R1, R2)
#define MOVE_MOV(d, s) "v_mov_b32 " d ", " s "\n\t"
#define MOVE_ADD(d, s) "v_add_u32 " d ", 0, " s "\n\t"
#define E_TWO_MOVES(MOVE, R1, R2, R3, P01, P23) MOVE(R2, R1) "v_mov_b32 " R3 ", 0\n\t"
#define E_SHIFT(MOVE, R1, R2, R3, P01, P23) "v_lshrrev_b64 " P23 ", 32, " P01 "\n\t"
#define SET_A "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v[40:41]", "v[42:43]", "v[44:45]", "s[80:81]"
#define SET_B "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v[48:49]", "v[50:51]", "v[52:53]", "s[86:87]"
#define PAIR_OLD(first) ASM_OLD(first, SET_A) ASM_OLD("v40", "v41", "v44", "v45", SET_B)
#define PAIR_CHAIN(MOVE, ZERO_E, first) ASM_CHAIN(MOVE, ZERO_E, first, SET_A) ASM_CHAIN(MOVE, ZERO_E, "v40", "v41", "v44", "v45", SET_B)
#define FROM_OPS "%0", "%1", "%2", "%3"
#define FROM_B "v48", "v49", "v52", "v53"
#define X2(a, b) a b
#define X16(first, rest) X2(first, rest) X2(rest, rest) X2(rest, rest) X2(rest, rest) X2(rest, rest) X2(rest, rest) X2(rest, rest) X2(rest, rest)
#define KERNEL_PRODUCT(name, FIRST, REST) \
    __global__ void __launch_bounds__(1024) name(uint32_t* out, Stamp* stamps, uint32_t seed) { \
        PROLOGUE \
        asm volatile(X16(FIRST, REST) "v_mov_b32 %0, v48\n\tv_mov_b32 %1, v49\n\tv_mov_b32 %2, v52\n\tv_mov_b32 %3, v53" \
                     : "+v"(a[0]), "+v"(b[0]), "+v"(c[0]), "+v"(d[0]) \
                     : : "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "vcc", "s80", "s81", "s86", "s87"); \
        EPILOGUE }
KERNEL_PRODUCT(k_product_old, PAIR_OLD(FROM_OPS), PAIR_OLD(FROM_B))
KERNEL_PRODUCT(k_product_chain_mov, PAIR_CHAIN(MOVE_MOV, E_TWO_MOVES, FROM_OPS), PAIR_CHAIN(MOVE_MOV, E_TWO_MOVES, FROM_B))
KERNEL_PRODUCT(k_product_chain_add, PAIR_CHAIN(MOVE_ADD, E_TWO_MOVES, FROM_OPS), PAIR_CHAIN(MOVE_ADD, E_TWO_MOVES, FROM_B))
KERNEL_PRODUCT(k_product_chain_shift, PAIR_CHAIN(MOVE_MOV, E_SHIFT, FROM_OPS), PAIR_CHAIN(MOVE_MOV, E_SHIFT, FROM_B))
// ---- round 8: the carry's correction c (2^32 - 1) behind every reduction as ONE multiply-add (t = c ? 1 : 0;  r = t (2^32 - 1) + r) against
// the select of 0 / -1 + 64-bit addition it replaces; measured on the whole reduction tail of csrc/gl.h, the whole fold96 of csrc/poseidon.h and
// the whole product, each as a block whose result is the next block's operand, 32 blocks per loop iteration, in place on fixed registers
// (v40..v47 scratch as in gl.h, v48..v51 the product's operands; 4 moves in and 4 out per iteration, the same for every form: ~1 %).
// SEL makes t from the carry in s[80:81] (the tail) or vcc (fold96).
#define R8_SEL_MINUS1(S) "v_cndmask_b32_e64 v47, 0, -1, " S "\n\t"
#define R8_SEL_CNDMASK(S) "v_cndmask_b32_e64 v47, 0, 1, " S "\n\t"
#define R8_SEL_ADDC(S) "v_addc_co_u32_e64 v47, " S ", 0, 0, " S "\n\t"
#define R8_ADD_OLD(O0, O1, OP) "v_add_co_u32_e32 " O0 ", vcc, v40, v47\n\tv_addc_co_u32_e64 " O1 ", vcc, v41, 0, vcc\n\t"
#define R8_ADD_MAD(O0, O1, OP) "v_mad_u64_u32 " OP ", vcc, v47, -1, v[40:41]\n\t"
// the tail: 128-bit value {v[40:41], v44, v45} -> a residue in (O0, O1) = the pair OP.  SUB0: the first word of u - hi_hi (with or without borrow-in)
#define R8_SUB0_PLAIN "v_sub_co_u32_e32 v40, vcc, v40, v45\n\t"
#define R8_SUB0_BORROW_IN "v_subb_co_u32_e64 v40, vcc, v40, v45, s[82:83]\n\t"
#define R8_TAIL(SEL, ADD, SUB0, O0, O1, OP) \
    "v_mad_u64_u32 v[40:41], s[80:81], v44, -1, v[40:41]\n\t" \
    SUB0 \
    "v_subbrev_co_u32_e32 v41, vcc, 0, v41, vcc\n\t" \
    SEL("s[80:81]") \
    "s_cbranch_vccz 1f\n\t" \
    "v_cndmask_b32_e64 v46, 0, -1, vcc\n\t" \
    "v_sub_co_u32_e32 v40, vcc, v40, v46\n\t" \
    "v_subbrev_co_u32_e32 v41, vcc, 0, v41, vcc\n" \
    "1:\n\t" \
    ADD(O0, O1, OP)
// fold96: acc_lo = v[40:41] (in and out), hi_lo = v44, hi_hi = v45
#define R8_FOLD(SEL, ADD) \
    "v_mad_u64_u32 v[40:41], vcc, v45, -1, v[40:41]\n\t" \
    "v_add_co_u32_e32 v41, vcc, v41, v44\n\t" \
    SEL("vcc") \
    ADD("v40", "v41", "v[40:41]")
// the product a (v48, v49) x b (v50, v51) chained as in gl.h; CARRY the SGPR pair of the middle word's carry c_M, F1 what makes F's high word
#define R8_PRODUCT(CARRY, F1) \
    "v_mad_u64_u32 v[40:41], vcc, v48, v50, 0\n\t" \
    "v_lshrrev_b64 v[42:43], 32, v[40:41]\n\t" \
    "v_mad_u64_u32 v[42:43], vcc, v48, v51, v[42:43]\n\t" \
    "v_mad_u64_u32 v[42:43], " CARRY ", v49, v50, v[42:43]\n\t" \
    "v_mov_b32 v44, v43\n\t" \
    F1 \
    "v_mad_u64_u32 v[44:45], vcc, v49, v51, v[44:45]\n\t" \
    "v_mov_b32 v41, v42\n\t"
#define R8_F1_CARRY "v_cndmask_b32_e64 v45, 0, 1, s[80:81]\n\t"
#define R8_F1_ZERO "v_mov_b32 v45, 0\n\t"
#define X32(b) X16(X2(b, b), X2(b, b))
#define KERNEL_R8(name, V0, V1, V2, V3, BLOCK) \
    __global__ void __launch_bounds__(1024) name(uint32_t* out, Stamp* stamps, uint32_t seed) { \
        PROLOGUE \
        asm volatile("v_mov_b32 " V0 ", %0\n\tv_mov_b32 " V1 ", %1\n\tv_mov_b32 " V2 ", %2\n\tv_mov_b32 " V3 ", %3\n\t" \
                     X32(BLOCK) \
                     "v_mov_b32 %0, " V0 "\n\tv_mov_b32 %1, " V1 "\n\tv_mov_b32 %2, " V2 "\n\tv_mov_b32 %3, " V3 \
                     : "+v"(a[0]), "+v"(b[0]), "+v"(c[0]), "+v"(d[0]) \
                     : : "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "vcc", "scc", "s80", "s81", "s82", "s83"); \
        EPILOGUE }
#define KERNEL_R8_RED(name, BLOCK) KERNEL_R8(name, "v40", "v41", "v44", "v45", BLOCK)
#define KERNEL_R8_MUL(name, BLOCK) KERNEL_R8(name, "v48", "v49", "v50", "v51", BLOCK)
KERNEL_R8_RED(k_tail_old, R8_TAIL(R8_SEL_MINUS1, R8_ADD_OLD, R8_SUB0_PLAIN, "v40", "v41", "v[40:41]"))
KERNEL_R8_RED(k_tail_mad_cndmask, R8_TAIL(R8_SEL_CNDMASK, R8_ADD_MAD, R8_SUB0_PLAIN, "v40", "v41", "v[40:41]"))
KERNEL_R8_RED(k_tail_mad_addc, R8_TAIL(R8_SEL_ADDC, R8_ADD_MAD, R8_SUB0_PLAIN, "v40", "v41", "v[40:41]"))
KERNEL_R8_RED(k_fold_old, R8_FOLD(R8_SEL_MINUS1, R8_ADD_OLD))
KERNEL_R8_RED(k_fold_mad_cndmask, R8_FOLD(R8_SEL_CNDMASK, R8_ADD_MAD))
KERNEL_R8_RED(k_fold_mad_addc, R8_FOLD(R8_SEL_ADDC, R8_ADD_MAD))
KERNEL_R8_MUL(k_mul_old, R8_PRODUCT("s[80:81]", R8_F1_CARRY) R8_TAIL(R8_SEL_MINUS1, R8_ADD_OLD, R8_SUB0_PLAIN, "v48", "v49", "v[48:49]"))
KERNEL_R8_MUL(k_mul_mad_cndmask, R8_PRODUCT("s[80:81]", R8_F1_CARRY) R8_TAIL(R8_SEL_CNDMASK, R8_ADD_MAD, R8_SUB0_PLAIN, "v48", "v49", "v[48:49]"))
KERNEL_R8_MUL(k_mul_mad_addc, R8_PRODUCT("s[80:81]", R8_F1_CARRY) R8_TAIL(R8_SEL_ADDC, R8_ADD_MAD, R8_SUB0_PLAIN, "v48", "v49", "v[48:49]"))
// add_a: a (v40, v41, in and out) + b (v44, v45) for any residues; the second correction sits behind its never-taken wave-level branch
#define R8_ADDA_OLD \
    "v_add_co_u32_e32 v40, vcc, v40, v44\n\t" \
    "v_addc_co_u32_e32 v41, vcc, v41, v45, vcc\n\t" \
    "v_cndmask_b32_e64 v47, 0, -1, vcc\n\t" \
    "v_add_co_u32_e32 v40, vcc, v40, v47\n\t" \
    "v_addc_co_u32_e64 v41, vcc, 0, v41, vcc\n\t" \
    "s_cbranch_vccz 1f\n\t" \
    "v_cndmask_b32_e64 v47, 0, -1, vcc\n\t" \
    "v_add_co_u32_e32 v40, vcc, v40, v47\n\t" \
    "v_addc_co_u32_e64 v41, vcc, 0, v41, vcc\n" \
    "1:\n\t"
#define R8_ADDA_MAD \
    "v_add_co_u32_e32 v42, vcc, v40, v44\n\t" \
    "v_addc_co_u32_e32 v43, vcc, v41, v45, vcc\n\t" \
    "v_cndmask_b32_e64 v47, 0, 1, vcc\n\t" \
    "v_mad_u64_u32 v[40:41], vcc, v47, -1, v[42:43]\n\t" \
    "s_cbranch_vccz 1f\n\t" \
    "v_cndmask_b32_e64 v47, 0, 1, vcc\n\t" \
    "v_mad_u64_u32 v[40:41], vcc, v47, -1, v[40:41]\n" \
    "1:\n\t"
KERNEL_R8_RED(k_adda_old, R8_ADDA_OLD)
KERNEL_R8_RED(k_adda_mad, R8_ADDA_MAD)
// c_M as the borrow-in of u - hi_hi (weight 2^96 = -1): F = {M.hi, 0}, one more live scalar pair (s[82:83])
KERNEL_R8_MUL(k_mul_mad_cndmask_cm, R8_PRODUCT("s[82:83]", R8_F1_ZERO) R8_TAIL(R8_SEL_CNDMASK, R8_ADD_MAD, R8_SUB0_BORROW_IN, "v48", "v49", "v[48:49]"))
typedef void (*kern_t)(uint32_t*, Stamp*, uint32_t);
struct Entry {
    const char* name;
    kern_t k;
    int instr_per_body;   // wave instructions per chain step
    bool per_block;       // report cycles per chain step (a whole product assembly), not per instruction
};

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : nullptr;   // rows whose name contains this text (repeated runs of a few rows)
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("device %s, %d CUs, nominal clock %d kHz, LDS per CU %zu\n", prop.gcnArchName, cus, prop.clockRate, prop.maxSharedMemoryPerMultiProcessor);
    const Entry es[] = {
        {"v_fma_f32", k_fma_f32, 1}, {"v_pk_fma_f32 (2 FMA/lane)", k_pk_fma_f32, 1}, {"v_fma_f64", k_fma_f64, 1}, {"v_add_u32", k_add_u32, 1},
        {"v_xor_b32", k_xor_b32, 1}, {"v_and_or_b32", k_and_or_b32, 1}, {"v_add3_u32", k_add3_u32, 1}, {"v_mul_lo_u32", k_mul_lo_u32, 1},
        {"v_mul_hi_u32", k_mul_hi_u32, 1}, {"v_mad_u32_u24", k_mad_u32_u24, 1}, {"v_mad_u64_u32 (vgpr x vgpr)", k_mad_u64_u32, 1},
        {"v_mad_u64_u32 (vgpr x sgpr)", k_mad_u64_u32_s, 1}, {"v_add_co_u32_e64", k_add_co_u32, 1}, {"add_u64 (add_co+addc)", k_add_u64, 2},
        {"v_lshl_add_u64", k_lshl_add_u64, 1}, {"v_cndmask_b32_e64", k_cndmask, 1}, {"v_lshlrev_b64", k_lshlrev_b64, 1},
        {"v_alignbit_b32", k_alignbit, 1}, {"mix: mad_u64_u32 + add_co", k_mix_poseidon, 2},
        {"v_mov_b32", k_mov_b32, 1}, {"v_add_u32 dst, 0, src", k_add_u32_mov, 1}, {"v_cndmask_b32_e32 (vcc)", k_cndmask_e32, 1},
        {"v_cndmask_b32_e32 0, x, vcc", k_cndmask_e32_const, 1}, {"v_add_co_u32_e32 (vcc)", k_add_co_e32, 1}, {"v_addc_co_u32_e32 (vcc)", k_addc_co_e32, 1}, {"v_lshrrev_b64 by 32", k_lshrrev_b64_32, 1},
        {"mix: 2 mad_u64_u32 + add_u32", k_mix_mad2_add, 3},
        {"product: old (8 half)", k_product_old, 1, true}, {"product: chained, v_mov (5+4)", k_product_chain_mov, 1, true},
        {"product: chained, v_add (5+4)", k_product_chain_add, 1, true}, {"product: chained, shift (6+2)", k_product_chain_shift, 1, true},
        // round 8 (32 blocks per loop iteration, as the product rows)
        {"r8 tail: 0/-1 + add64 (6)", k_tail_old, 1, true}, {"r8 tail: cndmask 0/1 + mad (5)", k_tail_mad_cndmask, 1, true},
        {"r8 tail: addc 0/1 + mad (5)", k_tail_mad_addc, 1, true}, {"r8 fold96: 0/-1 + add64 (5)", k_fold_old, 1, true},
        {"r8 fold96: cndmask 0/1+mad (4)", k_fold_mad_cndmask, 1, true}, {"r8 fold96: addc 0/1 + mad (4)", k_fold_mad_addc, 1, true},
        {"r8 mul_nc: as it was (12+2)", k_mul_old, 1, true}, {"r8 mul_nc: cndmask+mad (11+2)", k_mul_mad_cndmask, 1, true},
        {"r8 mul_nc: addc + mad (11+2)", k_mul_mad_addc, 1, true}, {"r8 mul_nc: c_M borrow-in(10+3)", k_mul_mad_cndmask_cm, 1, true},
        {"r8 add_a: 0/-1 + add64 (5)", k_adda_old, 1, true}, {"r8 add_a: cndmask 0/1+mad (4)", k_adda_mad, 1, true},
    };
    const int ws[] = {1, 2, 4, 8};
    const size_t max_threads = (size_t)cus * 2048;
    uint32_t* d_out;
    Stamp* d_st;
    CHECK(hipMalloc(&d_out, max_threads * 4));
    CHECK(hipMalloc(&d_st, max_threads / 64 * sizeof(Stamp)));
    std::vector<Stamp> st(max_threads / 64);
    hipEvent_t ev0, ev1;
    CHECK(hipEventCreate(&ev0));
    CHECK(hipEventCreate(&ev1));
    printf("rows named product: cycles of one SIMD per whole assembly of the 128-bit product (a block of dependent instructions)\n");
    printf("cycles of one SIMD per wave64 instruction: in-kernel span of the SIMD's waves / from the HIP-event time of the launch\n");
    printf("%-30s", "");
    for (int w : ws) printf("  w=%d per SIMD", w);
    printf("   sclk(GHz)\n");
    for (const Entry& e : es) {
        if (only && !strstr(e.name, only)) continue;
        printf("%-30s", e.name);
        double ghz = 0;
        for (int w : ws) {
            // one workgroup per CU (w <= 4) or two (w = 8): the LDS request makes a second (third) workgroup not fit
            const int threads = w <= 4 ? 256 * w : 1024;
            const int per_cu = w <= 4 ? 1 : 2;
            const size_t lds = w <= 4 ? 96 * 1024 : 64 * 1024;
            CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(e.k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            const int blocks = cus * per_cu;
            double best = 1e30, evt = 0;
            for (int rep = 0; rep < 4; ++rep) {
                CHECK(hipEventRecord(ev0));
                hipLaunchKernelGGL(e.k, dim3(blocks), dim3(threads), lds, 0, d_out, d_st, 7u + rep);
                CHECK(hipEventRecord(ev1));
                CHECK(hipDeviceSynchronize());
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, ev0, ev1));
                const size_t waves = (size_t)blocks * threads / 64;
                CHECK(hipMemcpy(st.data(), d_st, waves * sizeof(Stamp), hipMemcpyDeviceToHost));
                // group the waves by the SIMD that ran them (XCC, SE, SH, CU, SIMD): one SIMD's throughput = the instructions of all its
                // waves / the span from its first start to its last end (s_memtime of one SIMD's waves is one clock domain); waves of a
                // SIMD need not run in lock-step (issue arbitration prefers the older wave), so a per-wave time would mislead
                std::map<uint64_t, std::array<double, 4>> simd;   // key -> {min c0, max c1, waves, sum of per-wave clock}
                for (size_t i = 0; i < waves; ++i) {
                    const uint32_t h = st[i].hw_id;
                    const uint64_t key = ((uint64_t)(st[i].xcc_id & 0xF) << 32) | (h & 0xFF30);   // se_id[15:13] sh_id[12] cu_id[11:8] simd_id[5:4]
                    auto it = simd.find(key);
                    const double clk = (double)(st[i].c1 - st[i].c0) / ((double)(st[i].r1 - st[i].r0) * 10.0);   // s_memrealtime: 100 MHz
                    if (it == simd.end()) simd[key] = {(double)st[i].c0, (double)st[i].c1, 1.0, clk};
                    else {
                        it->second[0] = std::min(it->second[0], (double)st[i].c0);
                        it->second[1] = std::max(it->second[1], (double)st[i].c1);
                        it->second[2] += 1.0;
                        it->second[3] += clk;
                    }
                }
                std::vector<double> per, clks;
                size_t uneven = 0;
                for (auto& kv : simd) {
                    if ((int)kv.second[2] != w) ++uneven;
                    per.push_back((kv.second[1] - kv.second[0]) / ((double)ITERS * CHAINS * REPS * e.instr_per_body * kv.second[2]));
                    clks.push_back(kv.second[3] / kv.second[2]);
                }
                std::nth_element(per.begin(), per.begin() + per.size() / 2, per.end());
                std::nth_element(clks.begin(), clks.begin() + clks.size() / 2, clks.end());
                const double per_instr = per[per.size() / 2];
                if (rep == 1 && (simd.size() != (size_t)cus * 4 || uneven)) printf("[%zu SIMDs seen, %zu without exactly %d waves] ", simd.size(), uneven, w);
                if (rep > 0 && per_instr < best) {
                    best = per_instr;
                    ghz = clks[clks.size() / 2];
                    // cross-check from outside the kernel: HIP-event time of the whole launch (launch overhead and tail included) at the
                    // clock the waves measured
                    evt = ms * 1e-3 * ghz * 1e9 / ((double)ITERS * CHAINS * REPS * e.instr_per_body * w);
                }
            }
            printf("  %5.2f/%5.2f", best, evt);
        }
        printf("   %8.3f\n", ghz);
    }
    return 0;
}

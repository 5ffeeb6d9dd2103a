// The reductions of csrc/gl.h and csrc/poseidon.h whose carry correction is one multiply-add (reduce128_asm, reduce96_asm, the tail of mul_nc /
// mul2_nc / dot2_nc / mad_nc, add_a, fold96) and the two shapes of the permutation built on them, run on operands read from a file, results written to a
// file: the caller (tests/test_gpu_reductions.py) owns the operands, their classes and the big-integer reference.  Element i is thread i of
// 256-thread blocks, so 64 consecutive elements starting at a multiple of 64 are one wave (the rare corrections sit behind wave-level branches).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/test_reductions.hip -o tools/test_reductions
//   test_reductions red IN OUT    IN = lo[n] hi_lo[n] hi_hi[n] (u64 each, the high words < 2^32);  OUT = canon of reduce128_asm(lo, hi_lo, hi_hi) |
//                                 reduce96_asm(lo, hi_lo), n words each
//   test_reductions forms IN OUT  IN = a[n] b[n] c[n] d[n];  OUT = canon of  a b | a b, c d (mul2_nc) | a b + c d | a b + c | a + b (add_a),
//                                 n words each
//   test_reductions fold IN OUT   IN = acc_lo[n] acc_hi[n];  OUT = canon of fold96(acc_lo, acc_hi), n words
//   test_reductions perm IN OUT   IN = n states of 12 words;  OUT = permute on the device (one lane each) | permute_wide (16 lanes each) | permute on
//                                 the host (the C form of the same header, which has no asm), 12 n words each
#include "../verifiable-fhe-paper_amd/csrc/poseidon.h"
#include <cstdio>
#include <cstring>
#include <vector>
using gl::u32;
using gl::u64;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__global__ void __launch_bounds__(256) k_red(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    const u64 lo = in[i];
    const u32 hi_lo = (u32)in[n + i], hi_hi = (u32)in[2 * n + i];
    out[i] = gl::canon(gl::reduce128_asm(lo, hi_lo, hi_hi));
    out[n + i] = gl::canon(gl::reduce96_asm(lo, hi_lo));
}
__global__ void __launch_bounds__(256) k_forms(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    const u64 a = in[i], b = in[n + i], c = in[2 * n + i], d = in[3 * n + i];
    out[i] = gl::canon(gl::mul_nc(a, b));
    u64 r, q;
    gl::mul2_nc(a, b, c, d, r, q);
    out[n + i] = gl::canon(r);
    out[2 * n + i] = gl::canon(q);
    out[3 * n + i] = gl::canon(gl::dot2_nc(a, b, c, d));
    out[4 * n + i] = gl::canon(gl::mad_nc(a, b, c));
    out[5 * n + i] = gl::canon(gl::add_a(a, b));
}
__global__ void __launch_bounds__(256) k_fold(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) out[i] = gl::canon(poseidon::fold96(in[i], in[n + i]));
}
__global__ void __launch_bounds__(256) k_perm(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = in[12 * i + k];
    poseidon::permute(s);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[12 * i + k] = s[k];
}
// every wave calls permute_wide with all its 64 lanes; a group beyond n runs on zeros and stores nothing
__global__ void __launch_bounds__(256) k_perm_wide(const u64* in, u64* out, size_t n) {
    __shared__ u64 lds[(256 / poseidon::WIDE_LANES) * poseidon::WIDE_LDS_WORDS];
    const unsigned l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const size_t i = blockIdx.x * (size_t)(256 / 16) + g;
    const bool live = i < n && l < 12;
    u64 x = live ? in[12 * i + l] : 0;
    x = poseidon::permute_wide(x, lds + g * poseidon::WIDE_LDS_WORDS, l);
    if (live) out[12 * i + l] = x;
}

int main(int argc, char** argv) {
    if (argc != 4) { printf("usage: test_reductions red|forms|fold|perm IN OUT\n"); return 2; }
    const char* modes[] = {"red", "forms", "fold", "perm"};
    const size_t per_in[] = {3, 4, 2, 12}, per_out[] = {2, 6, 1, 36};
    int mode = -1;
    for (int i = 0; i < 4; ++i) if (!strcmp(argv[1], modes[i])) mode = i;
    if (mode < 0) { printf("unknown mode %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { printf("cannot read %s\n", argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t words = (size_t)ftell(f) / 8, per = per_in[mode];
    fseek(f, 0, SEEK_SET);
    if (words == 0 || words % per) { printf("%s: %zu words is no multiple of %zu\n", argv[2], words, per); return 2; }
    std::vector<u64> in(words);
    if (fread(in.data(), 8, words, f) != words) { printf("short read\n"); return 2; }
    fclose(f);
    const size_t n = words / per, out_words = per_out[mode] * n, dev_words = mode == 3 ? 24 * n : out_words;
    std::vector<u64> out(out_words);
    u64 *d_in, *d_out;
    CK(hipMalloc(&d_in, words * 8));
    CK(hipMalloc(&d_out, dev_words * 8));
    CK(hipMemcpy(d_in, in.data(), words * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xFF, dev_words * 8));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (mode == 0) hipLaunchKernelGGL(k_red, grid, block, 0, 0, d_in, d_out, n);
    else if (mode == 1) hipLaunchKernelGGL(k_forms, grid, block, 0, 0, d_in, d_out, n);
    else if (mode == 2) hipLaunchKernelGGL(k_fold, grid, block, 0, 0, d_in, d_out, n);
    else {
        hipLaunchKernelGGL(k_perm, grid, block, 0, 0, d_in, d_out, n);
        hipLaunchKernelGGL(k_perm_wide, dim3((unsigned)((n + 15) / 16)), block, 0, 0, d_in, d_out + 12 * n, n);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, dev_words * 8, hipMemcpyDeviceToHost));
    if (mode == 3)
        for (size_t i = 0; i < n; ++i) {
            u64 s[12];
            for (int k = 0; k < 12; ++k) s[k] = in[12 * i + k];
            poseidon::permute_host(s);
            for (int k = 0; k < 12; ++k) out[24 * n + 12 * i + k] = s[k];
        }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 8, out_words, f) != out_words) { printf("cannot write %s\n", argv[3]); return 2; }
    fclose(f);
    printf("REDUCTIONS_DONE %s %zu\n", argv[1], n);
    return 0;
}

// The hand-scheduled Goldilocks products of csrc/gl.h (mul_nc, mul2_nc, dot2_nc, mad_nc) and the two shapes of the Poseidon permutation built
// on them, run on operands read from a file, results written to a file: the caller (tests/test_gpu_products.py) owns the operands and the
// reference.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/test_products.hip -o tools/test_products
//   test_products forms IN OUT   IN = a[n] b[n] c[n] d[n] (u64 each);  OUT = canon of  a b | a b, c d (mul2_nc) | a b + c d | a b + c, n words each
//   test_products perm IN OUT    IN = n states of 12 words;            OUT = permute (one lane each) | permute_wide (16 lanes each), 12 n words each
#include "../verifiable-fhe-paper_amd/csrc/poseidon.h"
#include <cstdio>
#include <cstring>
#include <vector>
using gl::u64;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

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
    if (argc != 4) { printf("usage: test_products forms|perm IN OUT\n"); return 2; }
    const bool forms = !strcmp(argv[1], "forms");
    if (!forms && strcmp(argv[1], "perm")) { printf("unknown mode %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { printf("cannot read %s\n", argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t words = (size_t)ftell(f) / 8, per = forms ? 4 : 12;
    fseek(f, 0, SEEK_SET);
    if (words == 0 || words % per) { printf("%s: %zu words is no multiple of %zu\n", argv[2], words, per); return 2; }
    std::vector<u64> in(words);
    if (fread(in.data(), 8, words, f) != words) { printf("short read\n"); return 2; }
    fclose(f);
    const size_t n = words / per, out_words = forms ? 5 * n : 24 * n;
    std::vector<u64> out(out_words);
    u64 *d_in, *d_out;
    CK(hipMalloc(&d_in, words * 8));
    CK(hipMalloc(&d_out, out_words * 8));
    CK(hipMemcpy(d_in, in.data(), words * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xFF, out_words * 8));
    if (forms) {
        hipLaunchKernelGGL(k_forms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    } else {
        hipLaunchKernelGGL(k_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
        hipLaunchKernelGGL(k_perm_wide, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, 0, d_in, d_out + 12 * n, n);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost));
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 8, out_words, f) != out_words) { printf("cannot write %s\n", argv[3]); return 2; }
    fclose(f);
    printf("PRODUCTS_DONE %s %zu\n", argv[1], n);
    return 0;
}

// The layers of csrc/poseidon.h (mds_add_const with and without constants, partial_group3 and both forms of partial_group3_core, the closing group of
// four, the permutation's head with the row subsets of its last layer) and the lazy
// accumulator of csrc/gl.h (LazyAcc::mac, mac_v, reduce) run on operands read from a file, results written to a file: the caller
// (tests/test_gpu_layers.py, tests/test_layers_cpu.py through tests/layer_cases.py) owns the operands, their classes and the big-integer
// reference.  Element i is thread i of 256-thread blocks, so elements [64 k, 64 k + 64) are one wave.
// The round constants of mds_row / group_row and the multiplicand of LazyAcc::mac are SCALAR operands of the inline assembly: they are per-launch
// data here (kernel arguments, or loads with a wave-uniform index), never per-element columns -- a per-lane value in a scalar operand is read
// from the first lane for the whole wave.  So a file starts with the launch's header, and one call is one launch.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/test_layers.hip -o tools/test_layers
//   test_layers MODE IN OUT        the device forms
//   test_layers host MODE IN OUT   the plain C forms of the same headers (LazyAcc, which has none: the restatement below); calls no HIP function, so
//                                  it runs without a GPU
//   mds      IN = kc[12] | n states of 12 words;  OUT = canon of mds_add_const(s, kc) | canon of mds_add_const(s, nullptr), 12 n words each
//   group    IN = g | n records of 15 words: state[12], w[3];  OUT = canon of partial_group3(s, g), 12 n words | canon of
//            partial_group3_core<false>(s, g, nullptr, x_out) followed by x_out[2], 14 n words | the same of partial_group3_core<true>(s, g, w, x_out)
//   group4   IN = kvec[12] k2 k3 k4 | n records of 16 words: state[12], w[4];  OUT = canon of closing_group4_core<false>(s, G, nullptr), 12 n words |
//            canon of closing_group4_core<true>(s, G, w), 12 n words -- G = the header (constants of the launch, not the table's)
//   tail     IN = n states of 12 words (round 4's input);  OUT = canon after six groups of three + the closing group of four, 12 n words | canon
//            after seven groups of three + the plain round 25, 12 n words: both are round 26's input
//   perm     IN = n states of 12 words;  OUT = canon of permute_head + last_rows<0, 12>, 12 n words | canon of the digest rows s[0..4) of
//            permute_digest, 4 n words | canon of the capacity rows s[8..12) of permute_sponge between two full blocks, 4 n words
//   lazyv    IN = L | c[L][n] | a[L][n];  OUT = canon of reduce() after L calls of mac_v(c, a), n words
//   lazys    IN = L | a[L] | c[L][n];  OUT = the same through mac(c0, c1, a0, a1) with the launch's a
//   lazyred  IN = e[n] m[n] h[n] ce[n] cm[n] ch[n];  OUT = canon of LazyAcc{e, m, h, ce, cm, ch}.reduce(), n words
#include "../verifiable-fhe-paper_amd/csrc/poseidon.h"
#include <cstdio>
#include <cstring>
#include <vector>
using gl::u32;
using gl::u64;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct Consts { u64 v[12]; };

// the forms, one element each: shared by the kernels and the host leg
GL_HD void do_mds(const u64* in, u64* out, size_t n, size_t i, const u64* kc) {
    u64 s[12], t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = t[k] = in[12 * i + k];
    poseidon::mds_add_const(s, kc);
    poseidon::mds_add_const(t, nullptr);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        out[12 * i + k] = gl::canon(s[k]);
        out[12 * n + 12 * i + k] = gl::canon(t[k]);
    }
}
GL_HD void do_group(const u64* in, u64* out, size_t n, size_t i, int g) {
    u64 s[12], t[12], u[12], w[3], xt[2], xu[2];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = t[k] = u[k] = in[15 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = in[15 * i + 12 + k];
    poseidon::partial_group3(s, g);
    poseidon::partial_group3_core<false>(t, g, nullptr, xt);
    poseidon::partial_group3_core<true>(u, g, w, xu);
    u64* o1 = out + 12 * n + 14 * i;
    u64* o2 = out + 26 * n + 14 * i;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        out[12 * i + k] = gl::canon(s[k]);
        o1[k] = gl::canon(t[k]);
        o2[k] = gl::canon(u[k]);
    }
    o1[12] = xt[0], o1[13] = xt[1];
    o2[12] = xu[0], o2[13] = xu[1];
}
GL_HD void do_group4(const u64* in, u64* out, size_t n, size_t i, const poseidon::ClosingGroup& G) {
    u64 s[12], t[12], w[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = t[k] = in[16 * i + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = in[16 * i + 12 + k];
    poseidon::closing_group4_core<false>(s, G, nullptr);
    poseidon::closing_group4_core<true>(t, G, w);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        out[12 * i + k] = gl::canon(s[k]);
        out[12 * n + 12 * i + k] = gl::canon(t[k]);
    }
}
GL_HD void do_tail(const u64* in, u64* out, size_t n, size_t i) {
    u64 s[12], t[12], kc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = t[k] = in[12 * i + k];
    for (int g = 0; g < 6; ++g) poseidon::partial_group3(s, g);
    poseidon::closing_group4(s);
    for (int g = 0; g < 7; ++g) poseidon::partial_group3(t, g);
#pragma unroll
    for (int k = 0; k < 12; ++k) kc[k] = poseidon::rc(12 * (poseidon::HALF_FULL + poseidon::N_PARTIAL) + k);
    t[0] = poseidon::sbox(t[0]);
    poseidon::mds_add_const(t, kc);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        out[12 * i + k] = gl::canon(s[k]);
        out[12 * n + 12 * i + k] = gl::canon(t[k]);
    }
}
GL_HD void do_perm(const u64* in, u64* out, size_t n, size_t i) {
    u64 s[12], t[12], u[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = t[k] = u[k] = in[12 * i + k];
    poseidon::permute_head(s);
    poseidon::last_rows<0, 12>(s, poseidon::head_halves(s));
    poseidon::permute_digest(t);
    poseidon::permute_sponge(u, 16, [](unsigned) {});
#pragma unroll
    for (int k = 0; k < 12; ++k) out[12 * i + k] = gl::canon(s[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[12 * n + 4 * i + k] = gl::canon(t[k]);
        out[16 * n + 4 * i + k] = gl::canon(u[8 + k]);
    }
}
// gl::LazyAcc is device code (its multiply-adds are assembly, reduce() is a __device__ member) and gl.h holds no C form of it: the host leg runs
// this restatement -- the four multiply-adds with their wrap counters in plain C, and reduce() line by line over the host forms of
// gl::reduce128_asm and gl::sub_a.  It proves the operands, classes and references of the lazy modes where there is no GPU.
struct LazyAccC {
    u64 e, m, h;
    u32 ce, cm, ch;
    void mac(u32 c0, u32 c1, u32 a0, u32 a1) {
        u64 t = (u64)c0 * a0;
        e += t, ce += e < t;
        t = (u64)c0 * a1;
        m += t, cm += m < t;
        t = (u64)c1 * a0;
        m += t, cm += m < t;
        t = (u64)c1 * a1;
        h += t, ch += h < t;
    }
    void mac_v(u64 c, u64 a) { mac((u32)c, (u32)(c >> 32), (u32)a, (u32)(a >> 32)); }
    u64 reduce() const {
        const u64 lo = e + (m << 32);
        const u64 t = (m >> 32) + ce + (lo < e ? 1u : 0u);
        const u64 H = h + t;
        const u64 hh = (H >> 32) + cm;
        const u64 top = (u64)ch + (H < t ? 1u : 0u) + (hh >> 32);
        return gl::sub_a(gl::reduce128_asm(lo, (u32)H, (u32)hh), top << 32);
    }
};
// Acc = gl::LazyAcc in the kernels, LazyAccC in the host leg
template <class Acc> GL_HD u64 do_lazyv(const u64* c, const u64* a, size_t n, size_t i, u64 L) {
    Acc acc{0, 0, 0, 0, 0, 0};
    for (u64 j = 0; j < L; ++j) acc.mac_v(c[j * n + i], a[j * n + i]);
    return gl::canon(acc.reduce());
}
template <class Acc> GL_HD u64 do_lazys(const u64* a, const u64* c, size_t n, size_t i, u64 L) {
    Acc acc{0, 0, 0, 0, 0, 0};
    for (u64 j = 0; j < L; ++j) {
        const u64 cj = c[j * n + i], aj = a[j];   // a[j]: the same word for the whole launch
        acc.mac((u32)cj, (u32)(cj >> 32), (u32)aj, (u32)(aj >> 32));
    }
    return gl::canon(acc.reduce());
}
template <class Acc> GL_HD u64 do_lazyred(const u64* in, size_t n, size_t i) {
    const Acc acc{in[i], in[n + i], in[2 * n + i], (u32)in[3 * n + i], (u32)in[4 * n + i], (u32)in[5 * n + i]};
    return gl::canon(acc.reduce());
}

__global__ void __launch_bounds__(256) k_mds(const u64* in, u64* out, size_t n, Consts kc) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) do_mds(in, out, n, i, kc.v);
}
__global__ void __launch_bounds__(256) k_group(const u64* in, u64* out, size_t n, int g) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) do_group(in, out, n, i, g);
}
__global__ void __launch_bounds__(256) k_group4(const u64* in, u64* out, size_t n, poseidon::ClosingGroup G) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) do_group4(in, out, n, i, G);
}
__global__ void __launch_bounds__(256) k_tail(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) do_tail(in, out, n, i);
}
__global__ void __launch_bounds__(256) k_perm(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) do_perm(in, out, n, i);
}
__global__ void __launch_bounds__(256) k_lazyv(const u64* c, const u64* a, u64* out, size_t n, u64 L) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) out[i] = do_lazyv<gl::LazyAcc>(c, a, n, i, L);
}
__global__ void __launch_bounds__(256) k_lazys(const u64* __restrict__ a, const u64* __restrict__ c, u64* __restrict__ out, size_t n, u64 L) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) out[i] = do_lazys<gl::LazyAcc>(a, c, n, i, L);
}
__global__ void __launch_bounds__(256) k_lazyred(const u64* in, u64* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) out[i] = do_lazyred<gl::LazyAcc>(in, n, i);
}

int main(int argc, char** argv) {
    const bool host = argc == 5 && !strcmp(argv[1], "host");
    if (argc != 4 && !host) { printf("usage: test_layers [host] mds|group|lazyv|lazys|lazyred|group4|tail|perm IN OUT\n"); return 2; }
    const char* const* arg = argv + (host ? 2 : 1);
    const char* modes[] = {"mds", "group", "lazyv", "lazys", "lazyred", "group4", "tail", "perm"};
    int mode = -1;
    for (int i = 0; i < 8; ++i) if (!strcmp(arg[0], modes[i])) mode = i;
    if (mode < 0) { printf("unknown mode %s\n", arg[0]); return 2; }
    FILE* f = fopen(arg[1], "rb");
    if (!f) { printf("cannot read %s\n", arg[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t words = (size_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<u64> in(words);
    if (fread(in.data(), 8, words, f) != words) { printf("short read\n"); return 2; }
    fclose(f);
    // header, words per element of the body and of the result
    size_t head = 0, per = 0, per_out = 1;
    u64 L = 0;
    if (mode == 0) head = 12, per = 12, per_out = 24;
    else if (mode == 1) head = 1, per = 15, per_out = 40;
    else if (mode == 4) head = 0, per = 6;
    else if (mode == 5) head = 15, per = 16, per_out = 24;
    else if (mode == 6) head = 0, per = 12, per_out = 24;
    else if (mode == 7) head = 0, per = 12, per_out = 20;
    else {
        if (words < 1 || in[0] == 0 || in[0] > (1u << 20)) { printf("%s: bad term count\n", arg[1]); return 2; }
        L = in[0];
        head = mode == 2 ? 1 : 1 + (size_t)L;
        per = mode == 2 ? 2 * (size_t)L : (size_t)L;
    }
    if (words <= head || (words - head) % per) { printf("%s: %zu words: no header of %zu and records of %zu\n", arg[1], words, head, per); return 2; }
    if (mode == 1 && in[0] > 6) { printf("%s: group %llu\n", arg[1], (unsigned long long)in[0]); return 2; }
    const size_t n = (words - head) / per, out_words = per_out * n;
    const u64* b = in.data() + head;
    std::vector<u64> out(out_words);
    poseidon::ClosingGroup G{};
    if (mode == 5) {
        memcpy(G.kvec, in.data(), sizeof G.kvec);
        G.k2 = in[12], G.k3 = in[13], G.k4 = in[14];
    }
    if (host) {
        for (size_t i = 0; i < n; ++i) {
            if (mode == 0) do_mds(b, out.data(), n, i, in.data());
            else if (mode == 1) do_group(b, out.data(), n, i, (int)in[0]);
            else if (mode == 2) out[i] = do_lazyv<LazyAccC>(b, b + L * n, n, i, L);
            else if (mode == 3) out[i] = do_lazys<LazyAccC>(in.data() + 1, b, n, i, L);
            else if (mode == 4) out[i] = do_lazyred<LazyAccC>(b, n, i);
            else if (mode == 5) do_group4(b, out.data(), n, i, G);
            else if (mode == 6) do_tail(b, out.data(), n, i);
            else do_perm(b, out.data(), n, i);
        }
    } else {
        u64 *d_in, *d_out;
        CK(hipMalloc(&d_in, words * 8));
        CK(hipMalloc(&d_out, out_words * 8));
        CK(hipMemcpy(d_in, in.data(), words * 8, hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xFF, out_words * 8));
        const u64* d_b = d_in + head;
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (mode == 0) {
            Consts kc;
            memcpy(kc.v, in.data(), sizeof kc.v);
            hipLaunchKernelGGL(k_mds, grid, block, 0, 0, d_b, d_out, n, kc);
        } else if (mode == 1) hipLaunchKernelGGL(k_group, grid, block, 0, 0, d_b, d_out, n, (int)in[0]);
        else if (mode == 2) hipLaunchKernelGGL(k_lazyv, grid, block, 0, 0, d_b, d_b + L * n, d_out, n, L);
        else if (mode == 3) hipLaunchKernelGGL(k_lazys, grid, block, 0, 0, (const u64*)(d_in + 1), d_b, d_out, n, L);
        else if (mode == 4) hipLaunchKernelGGL(k_lazyred, grid, block, 0, 0, d_b, d_out, n);
        else if (mode == 5) hipLaunchKernelGGL(k_group4, grid, block, 0, 0, d_b, d_out, n, G);
        else if (mode == 6) hipLaunchKernelGGL(k_tail, grid, block, 0, 0, d_b, d_out, n);
        else hipLaunchKernelGGL(k_perm, grid, block, 0, 0, d_b, d_out, n);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost));
        CK(hipFree(d_in));
        CK(hipFree(d_out));
    }
    f = fopen(arg[2], "wb");
    if (!f || fwrite(out.data(), 8, out_words, f) != out_words) { printf("cannot write %s\n", arg[2]); return 2; }
    fclose(f);
    printf("LAYERS_DONE %s %zu\n", arg[0], n);
    return 0;
}

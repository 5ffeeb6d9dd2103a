// The witness checker on the device: vpbs_check_witness (witness.hip) with the wires in HBM.
//
// Layout (uploaded once, at vpbs_witness_checker_create):
//   gates [n_gates], the six CosetTables of gates::coset_tables, constants [n_constants_cols][n], copy pairs [n_copies][2];
//   rows  [..]: every row whose gate has constraints, grouped by gate instance (ascending rows within a group);
//   segs  [..]: groups cut into runs of at most 64 rows -- one wave evaluates one run, so a wave evaluates ONE gate kind and the dispatch
//               on it is a scalar branch (the tile kernel of gates.hip does the same per tile).
// Kernels: check_gate_rows (one lane per row) and check_copies (one lane per copy pair) fold every violation into one 64-bit atomicMin key:
//   gate row:  row << 32 | constraint index      (bit 63 clear: any gate violation wins over any copy violation)
//   copy pair: 1 << 63 | pair index
// so the minimum is the host checker's first violation: the lowest violating row, within it the lowest constraint, and only without one
// the lowest violated pair.  The key then travels to pinned memory behind the kernels; the host formats vpbs_check_witness's message.
//
// Arithmetic: the constraints are the evaluators of gates.h instantiated for a field type of this file, H64, whose operations are the
// CANONICAL gl:: forms the host checker runs (gl::add / gl::sub / gl::mul, mulc = gl::mul).  On canonical wires that is the field; on a
// non-canonical word (p, 2^64 - 1) the device computes exactly what the host computes -- the residue forms the prover's kernels use
// (add_a / mul_nc ...) would canonicalise some values the host leaves at p, and the verdicts would differ.  gl.h is included first and
// the H64 overloads are declared before gates.h, so that the qualified gl:: calls of its templates see them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gl.h"

namespace gates {
struct H64 {
    gl::u64 v;
};
GL_HD H64 mulc(H64 a, gl::u64 c) { return H64{gl::mul(a.v, c)}; }
}  // namespace gates
namespace gl {
GL_HD gates::H64 add(gates::H64 a, gates::H64 b) { return gates::H64{add(a.v, b.v)}; }
GL_HD gates::H64 sub(gates::H64 a, gates::H64 b) { return gates::H64{sub(a.v, b.v)}; }
GL_HD gates::H64 mul(gates::H64 a, gates::H64 b) { return gates::H64{mul(a.v, b.v)}; }
}  // namespace gl

#include "context.h"
#include "gates.h"
#include "witness_check.h"

namespace gates {
template <> struct Fld<H64> {
    static GL_HD H64 lift(u64 c) { return H64{c}; }
};
}  // namespace gates

namespace {
using vpbs::DeviceError;
using vpbs::report;
using u32 = uint32_t;
using u64 = uint64_t;
constexpr u64 NO_VIOLATION = ~0ull;
constexpr u64 COPY_BIT = 1ull << 63;
constexpr unsigned SEG_ROWS = 64;   // one wave
constexpr unsigned WAVES_PER_BLOCK = 4;

struct Seg {
    u32 gate, start, count, pad;   // rows[start .. start + count) all carry gates[gate]
};
struct Shape {
    u64 n;
    unsigned n_wires, first_const, n_const_cols;
    u64 pih[4];
};

// RowVars of vpbs_check_witness over H64
struct DevRowVars {
    const u64* __restrict__ wires;
    const u64* __restrict__ constants;
    const Shape& sh;
    u64 row;
    __device__ gates::H64 wire(unsigned i) const { return gates::H64{i < sh.n_wires ? wires[(u64)i * sh.n + row] : 0}; }
    __device__ gates::H64 constant(unsigned i) const {
        return gates::H64{sh.first_const + i < sh.n_const_cols ? constants[(u64)(sh.first_const + i) * sh.n + row] : 0};
    }
    __device__ u64 pi_hash(unsigned i) const { return sh.pih[i]; }
};
// the index of the first constraint whose value is non-zero (the host's `s.c[k] != 0`: raw words)
struct FirstSink {
    unsigned k = 0, first = ~0u;
    __device__ void push(gates::H64 x) {
        if (x.v != 0 && first == ~0u) first = k;
        ++k;
    }
};

__global__ __launch_bounds__(SEG_ROWS* WAVES_PER_BLOCK) void check_gate_rows(const Seg* __restrict__ segs, unsigned n_segs,
                                                                              const u32* __restrict__ rows, const vpbs_gate* __restrict__ gate_list,
                                                                              const gates::CosetTables* __restrict__ coset,
                                                                              const u64* __restrict__ wires, const u64* __restrict__ constants,
                                                                              Shape sh, unsigned long long* key) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x / SEG_ROWS);
    const unsigned si = blockIdx.x * WAVES_PER_BLOCK + wave;   // wave-uniform
    if (si >= n_segs) return;
    const Seg sg = segs[si];
    const unsigned lane = threadIdx.x % SEG_ROWS;
    if (lane >= sg.count) return;
    const vpbs_gate g = gate_list[sg.gate];
    const u64 row = rows[sg.start + lane];
    const DevRowVars v{wires, constants, sh, row};
    FirstSink s;
    gates::eval_gate<gates::H64>(g, &coset[g.p0 <= 5 ? g.p0 : 0], v, s);
    if (s.first != ~0u) atomicMin(key, (unsigned long long)((row << 32) | s.first));
}

__global__ __launch_bounds__(256) void check_copies(const u32* __restrict__ copies, u64 n_copies, const u64* __restrict__ wires,
                                                    unsigned long long* key) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_copies) return;
    if (wires[copies[2 * i]] != wires[copies[2 * i + 1]]) atomicMin(key, (unsigned long long)(COPY_BIT | i));
}
}  // namespace

struct vpbs_witness_checker {
    vpbs_ctx* ctx = nullptr;
    unsigned log_n = 0, n_wires = 0, num_selectors = 0, n_const_cols = 0;
    size_t n = 0;
    // host copies: what the message of a violation needs
    std::vector<vpbs_gate> gates;
    std::vector<u32> row_gate, copies;
    // device tables
    vpbs_gate* d_gates = nullptr;
    gates::CosetTables* d_coset = nullptr;
    u64* d_constants = nullptr;
    u32 *d_rows = nullptr, *d_copies = nullptr;
    Seg* d_segs = nullptr;
    unsigned n_segs = 0;
    u64* d_key = nullptr;
    u64* d_stage = nullptr;           // host wires staged here (allocated at the first host run)
    volatile u64* h_key = nullptr;    // pinned: the key arrives here with the stream's next synchronisation
    std::vector<void*> owned;

    template <class T> T* upload(const T* h, size_t count) {
        T* d = static_cast<T*>(ctx->alloc_bytes(std::max<size_t>(1, count) * sizeof(T)));
        owned.push_back(d);
        if (count) VPBS_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return d;
    }
    ~vpbs_witness_checker() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
        if (h_key) (void)hipHostFree(const_cast<u64*>(h_key));
    }
};

namespace vpbs {
bool witness_check_fits(const vpbs_witness_checker* chk, const vpbs_ctx* ctx, unsigned log_n, unsigned n_wires) {
    return chk && ctx && chk->ctx->device == ctx->device && chk->log_n == log_n && chk->n_wires == n_wires;
}

void witness_check_enqueue(vpbs_witness_checker* chk, hipStream_t s, const u64* d_wires, const u64 pi_hash[4]) {
    Shape sh{chk->n, chk->n_wires, chk->num_selectors, chk->n_const_cols, {pi_hash[0], pi_hash[1], pi_hash[2], pi_hash[3]}};
    auto* key = reinterpret_cast<unsigned long long*>(chk->d_key);
    VPBS_HIP(hipMemsetAsync(chk->d_key, 0xFF, sizeof(u64), s));
    {
        Timed t(chk->ctx, "witness_check");
        if (chk->n_segs)
            check_gate_rows<<<(chk->n_segs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, SEG_ROWS * WAVES_PER_BLOCK, 0, s>>>(
                chk->d_segs, chk->n_segs, chk->d_rows, chk->d_gates, chk->d_coset, d_wires, chk->d_constants, sh, key);
        const size_t nc = chk->copies.size() / 2;
        if (nc) check_copies<<<(unsigned)((nc + 255) / 256), 256, 0, s>>>(chk->d_copies, nc, d_wires, key);
    }
    VPBS_HIP(hipGetLastError());
    *chk->h_key = 0;   // overwritten by the copy; NO_VIOLATION only if the kernels found nothing
    VPBS_HIP(hipMemcpyAsync(const_cast<u64*>(chk->h_key), chk->d_key, sizeof(u64), hipMemcpyDeviceToHost, s));
}

bool witness_check_result(const vpbs_witness_checker* chk, std::string& msg) {
    const u64 key = *chk->h_key;
    if (key == NO_VIOLATION) return true;
    const size_t n = chk->n;
    if (key & COPY_BIT) {
        const size_t i = (size_t)(key & ~COPY_BIT);
        const u32 a = chk->copies[2 * i], b = chk->copies[2 * i + 1];
        msg = "copy constraint violated: (column " + std::to_string(a / n) + ", row " + std::to_string(a % n) + ") != (column " +
              std::to_string(b / n) + ", row " + std::to_string(b % n) + ")";
    } else {
        const size_t r = (size_t)(key >> 32);
        const unsigned k = (unsigned)(key & 0xFFFFFFFFu);
        char id[256] = "gate";
        (void)vpbs_gate_id(&chk->gates[chk->row_gate[r]], id, sizeof id);
        id[60] = 0;
        msg = "row " + std::to_string(r) + ": constraint " + std::to_string(k) + " of " + id + " is not satisfied";
    }
    return false;
}
}  // namespace vpbs

extern "C" {
int vpbs_witness_checker_create(vpbs_ctx* ctx, const vpbs_circuit* c, vpbs_witness_checker** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    // vpbs_check_witness's argument checks (the generators are not read by a check)
    bool ok = ctx && out && c && c->gates && c->n_gates && c->row_gate && c->log_n >= 1 && c->log_n <= 24 && c->n_routed <= c->n_wires &&
              (!c->n_copies || c->copies);
    const size_t n = ok ? (size_t)1 << c->log_n : 0;
    for (size_t r = 0; ok && r < n; ++r) ok = c->row_gate[r] < c->n_gates;
    for (size_t i = 0; ok && i < 2 * c->n_copies; ++i) ok = c->copies[i] < (size_t)c->n_routed * n;
    for (unsigned i = 0; ok && i < c->n_gates; ++i) ok = c->gates[i].num_wires <= c->n_wires;
    if (!ok) {
        report(err, err_len, "malformed circuit description");
        return VPBS_ERR_INVALID;
    }
    unsigned max_consts = 0;
    for (unsigned i = 0; i < c->n_gates; ++i) max_consts = std::max(max_consts, c->gates[i].num_constants);
    if (c->num_selectors + max_consts > c->n_constants_cols || (max_consts && !c->constants)) {
        report(err, err_len, "constants columns missing");
        return VPBS_ERR_INVALID;
    }
    auto* k = new vpbs_witness_checker;
    k->ctx = ctx;
    k->log_n = c->log_n;
    k->n_wires = c->n_wires;
    k->num_selectors = c->num_selectors;
    k->n_const_cols = c->constants ? c->n_constants_cols : 0;
    k->n = n;
    k->gates.assign(c->gates, c->gates + c->n_gates);
    k->row_gate.assign(c->row_gate, c->row_gate + n);
    k->copies.assign(c->copies, c->copies + 2 * c->n_copies);
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        // rows grouped by gate instance, cut into runs of one wave
        std::vector<std::vector<u32>> by_gate(c->n_gates);
        for (size_t r = 0; r < n; ++r)
            if (c->gates[c->row_gate[r]].num_constraints) by_gate[c->row_gate[r]].push_back((u32)r);
        std::vector<u32> rows;
        std::vector<Seg> segs;
        for (u32 g = 0; g < c->n_gates; ++g) {
            const size_t base = rows.size();
            for (size_t i = 0; i < by_gate[g].size(); i += SEG_ROWS)
                segs.push_back(Seg{g, (u32)(base + i), (u32)std::min<size_t>(SEG_ROWS, by_gate[g].size() - i), 0});
            rows.insert(rows.end(), by_gate[g].begin(), by_gate[g].end());
        }
        gates::CosetTables tables[6];
        for (unsigned b = 0; b < 6; ++b) tables[b] = gates::coset_tables(b);
        k->d_gates = k->upload(c->gates, c->n_gates);
        k->d_coset = k->upload(tables, 6);
        k->d_constants = k->upload(c->constants, (size_t)k->n_const_cols * n);
        k->d_rows = k->upload(rows.data(), rows.size());
        k->d_segs = k->upload(segs.data(), segs.size());
        k->n_segs = (unsigned)segs.size();
        k->d_copies = k->upload(c->copies, 2 * c->n_copies);
        k->d_key = static_cast<u64*>(ctx->alloc_bytes(sizeof(u64)));
        k->owned.push_back(k->d_key);
        void* pinned = nullptr;
        VPBS_HIP(hipHostMalloc(&pinned, sizeof(u64), hipHostMallocDefault));
        k->h_key = static_cast<volatile u64*>(pinned);
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // the host vectors above go out of scope
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        report(err, err_len, e.what);
        delete k;
        return e.status;
    }
    *out = k;
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_witness_checker_free(vpbs_witness_checker* chk) { delete chk; }

int vpbs_witness_checker_run(vpbs_witness_checker* chk, const uint64_t* wires, int on_device, const uint64_t pi_hash[4], char* err,
                             size_t err_len) {
    if (!chk || !wires || !pi_hash) {
        report(err, err_len, "malformed circuit description");
        return VPBS_ERR_INVALID;
    }
    vpbs_ctx* ctx = chk->ctx;
    std::string msg;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const u64* d_wires = wires;
        if (!on_device) {
            const size_t words = (size_t)chk->n_wires * chk->n;
            if (!chk->d_stage) {
                chk->d_stage = ctx->alloc_words(words);
                chk->owned.push_back(chk->d_stage);
            }
            VPBS_HIP(hipMemcpyAsync(chk->d_stage, wires, words * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
            d_wires = chk->d_stage;
        }
        vpbs::witness_check_enqueue(chk, ctx->stream, d_wires, pi_hash);
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        report(err, err_len, e.what);
        return e.status;
    }
    const bool ok = vpbs::witness_check_result(chk, msg);
    report(err, err_len, msg);
    return ok ? 1 : 0;
}
}  // extern "C"

// Programs of lookup gates on resident keys (vpbs_program, include/vpbs_prover.h): a netlist whose every gate is one bootstrap of a linear
// combination of earlier wires.  The object validates and levelises the description on the host and keeps it on the device twice: in the
// caller's gate order (verification combines all gates at once) and permuted level by level (evaluation walks the levels).
//
//   run     per level, per chunk of the Bootstrapper's max_batch gates, on the Bootstrapper's context's stream:
//             lwe_combine_kernel   wire table -> the chunk's gate inputs  [gates][n_lwe + 1]
//             gather_rows_kernel   testvs[gate_lut] -> the chunk's test vectors  [gates][N]
//             pbs_batch_kernel     (vpbs::bootstrapper_enqueue) -> out_ct, and lwe_out straight into the level's rows of the wire table
//           The wire table on the device is in the PERMUTED order, so a level's outputs are contiguous rows; gather_rows_kernel puts the
//           outputs back into the caller's order at the end.  The levels are ordered by the stream; nothing waits inside a kernel for
//           another workgroup; the host waits once.
//   run_batch  one program, `instances` input sets, instance b under the key set of slot key_of[b] of a key ring: level l of ALL instances
//           goes into key-ring launches of the ring's max_batch rows (vpbs::keyring_enqueue).  The wire table is level-major -- the
//           block of inputs [instances][n_inputs], then per level a block [instances][gates of the level] -- with the instances in slot
//           order (a stable sort of key_of on the host), so that a chunk of consecutive rows is grouped by key set and its lwe_out is a
//           contiguous piece of the level's block:
//             lwe_combine_batch_kernel   level-major wire table -> the chunk's gate inputs
//             gather_rows_kernel         testvs[gate_lut of the row] -> the chunk's test vectors
//             pbs_keyring_kernel         -> out_ct, and lwe_out straight into the level's block
//           Every index array of every launch is uploaded once, before the first launch; gather_rows_kernel delivers the three outputs in
//           the caller's instance and gate order; the host waits once.
//   prove   run on the batch prover's Bootstrapper, then vpbs_pbs_prover_run on the gate inputs (caller's order) with per-gate test vectors.
//   prove_batch  run_batch on the ring of a ring prover (pbs_prove_ring.hip), then vpbs_ring_prover_run on the gate inputs of every instance,
//           row b * n_gates + g under the slot of instance b, under the prover's mutex from the evaluation to the last proof.
//   verify  upload inputs and claimed outputs, lwe_extract_kernel on all outputs, ONE lwe_combine_kernel over all gates in the caller's
//           order, then vpbs_pbs_verifier_run in chunks.
//   verify_batch  verify for all instances on a ring verifier (verify_pbs_batch.hip): upload inputs and claimed outputs of ALL instances, ONE
//           lwe_extract_kernel, ONE lwe_combine_rows_kernel over the rows (instance, gate) in the caller's order, then per chunk of the ring
//           verifier's max_batch rows the verifier's core on device pointers into these tables (vpbs::pbs_verify_enqueue) -- the test
//           vector of a row through testv_of = gate_lut, the key hash through key_of of the row's instance; both index arrays are
//           uploaded once -- and one wait for the chunk's result bytes.
//   One proof per program instance: the gates of an instance are the leaves of ONE aggregate (aggregate.hip), in gate order.
//   gate_inputs, aggregate_root, verify_aggregate   the statement on the HOST (a host-only program will do): the wire table from the claimed
//           outputs (multi_lut::extract_at_word), lwe_combine_kernel's arithmetic and the snap in plain C++, then vpbs_aggregate_root /
//           vpbs_verify_aggregate over those gate inputs with testv_of = gate_lut.
//   prove_aggregate, prove_aggregate_batch   prove / prove_batch with the proofs kept, then vpbs_aggregator_run per instance, after the last proof.
//   verify_aggregate_batch   verify_batch's upload, ONE extraction launch and ONE lwe_combine_rows_kernel over all instances, then the tables
//           where they lie to vpbs_aggregate_verifier_run_many (device pointers; testv_of = gate_lut tiled, the key index per row), in chunks
//           of the verifier's max_aggregates / max_leaves on the same stream, one wait per chunk.
//
// Multi-output gates (vpbs_program_create_multi): gate g has outs[g] output wires and a snap of slots[g].  Everything above
// holds with "outputs of the level" for "gates of the level" in both wire tables; the gate inputs, the output GLWEs and the proofs stay
// per gate.  For such a program (multi): the combine kernels run in their SNAP instantiation, the bootstrap launch writes out_ct only,
// and ONE lwe_extract_at_kernel launch per chunk (multi_lut.hip) fills the chunk's output rows -- contiguous in both tables -- behind it on
// the same stream; verify and verify_batch extract all (gate, j) rows in one launch.  A description whose every gate is (0, 1) is not
// multi: it runs exactly the launches listed above.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "context.h"
#include "multi_lut.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::u64;
using u32 = uint32_t;

namespace vpbs {
namespace {
struct CombineArgs {
    const u64* wires;      // [n_wires][words]
    const u64* first;      // [n_gates + 1]
    const u32* src;        // [n_terms]: rows of `wires`
    const u64* coef;       // [n_terms]
    const u64* cst;        // [n_gates]
    u64* out;              // [count][words]: row 0 is gate `gate0`
    unsigned gate0, words; // words = n_lwe + 1
    const u32* slots;      // SNAP only: [n_gates], log2 of the gate's slots (multi_lut.h); log_n: of the ring
    unsigned log_n;
};

// One workgroup per gate, lanes on consecutive words of the ciphertext: every term is one coalesced read of a wire row.  The term list, the
// coefficients and the constant depend on blockIdx.x alone, so their loads are wave-uniform.  A wire word is reduced before it is used (an
// input ciphertext may hold words at or above p; bootstrap outputs are canonical); products and sums are canonical in, canonical out.
// SNAP (programs with multi-output gates): every word of the canonical sum is rounded by the gate's own slots_log before it is stored; the
// variant without it is the kernel as it was.
template <bool SNAP>
__global__ void __launch_bounds__(256) lwe_combine_kernel(CombineArgs a) {
    const unsigned g = a.gate0 + blockIdx.x;
    const u64 t0 = a.first[g], t1 = a.first[g + 1];
    const u64 c = a.cst[g];
    u64* out = a.out + (size_t)blockIdx.x * a.words;
    const unsigned sl = SNAP ? a.slots[g] : 0;
    for (unsigned j = threadIdx.x; j < a.words; j += 256) {
        u64 s = j + 1 == a.words ? c : 0;
        for (u64 t = t0; t < t1; ++t) s = gl::add(s, gl::mul(a.coef[t], gl::canon(a.wires[(size_t)a.src[t] * a.words + j])));
        out[j] = SNAP ? multi_lut::snap(s, a.log_n, sl) : s;
    }
}

struct CombineBatchArgs {
    const u64* wires;       // the level-major table of a batched evaluation
    const u64* first;       // [n_gates + 1], permuted order
    const u32* loc;         // [n_terms][3]: the source wire's block (first row per instance), the block's width, the position in it
    const u64* coef;        // [n_terms]
    const u64* cst;         // [n_gates]
    u64* out;               // [count][words]: row 0 is row `row0` of the level's block
    size_t instances;
    unsigned row0, gate0, width, words;   // gate0: the level's first permuted gate; width: gates of the level
    const u32* slots;       // SNAP only, as CombineArgs (permuted order)
    unsigned log_n;
};

// lwe_combine_kernel for the rows of one level of MANY instances: one workgroup per (instance, gate) row, lanes on consecutive words.  Row r
// of the level's block is gate gate0 + r % width of the instance at sorted position r / width; the term list, the coefficients, the
// constant and the source rows depend on blockIdx.x alone (wave-uniform), and a term is one coalesced read of a wire row.  The same
// arithmetic in the same order: canonical on read, canonical products and sums, the constant in the body only.  A term's block is a level's
// block of OUTPUT rows (as wide as the level has gates when every gate has one output); SNAP as in lwe_combine_kernel.
template <bool SNAP>
__global__ void __launch_bounds__(256) lwe_combine_batch_kernel(CombineBatchArgs a) {
    const unsigned r = a.row0 + blockIdx.x;
    const size_t inst = r / a.width;
    const unsigned g = a.gate0 + r % a.width;
    const u64 t0 = a.first[g], t1 = a.first[g + 1];
    const u64 c = a.cst[g];
    u64* out = a.out + (size_t)blockIdx.x * a.words;
    const unsigned sl = SNAP ? a.slots[g] : 0;
    for (unsigned j = threadIdx.x; j < a.words; j += 256) {
        u64 s = j + 1 == a.words ? c : 0;
        for (u64 t = t0; t < t1; ++t) {
            const u32* l = a.loc + 3 * t;
            const size_t row = a.instances * l[0] + inst * l[1] + l[2];
            s = gl::add(s, gl::mul(a.coef[t], gl::canon(a.wires[row * a.words + j])));
        }
        out[j] = SNAP ? multi_lut::snap(s, a.log_n, sl) : s;
    }
}

struct CombineRowsArgs {
    const u64* wires;       // [instances][n_in] input rows, then [instances][n_outs] gate-output rows
    const u64* first;       // [n_gates + 1], the caller's order
    const u32* src;         // [n_terms]: wires of the caller's numbering
    const u64* coef;        // [n_terms]
    const u64* cst;         // [n_gates]
    u64* out;               // [instances * n_gates][words]
    size_t instances;
    unsigned n_in, n_gates, words;
    unsigned n_outs;        // output wires per instance: n_gates when every gate has one
    const u32* slots;       // SNAP only, as CombineArgs (the caller's order)
    unsigned log_n;
};

// lwe_combine_kernel for ALL gates of MANY instances in the caller's order (verification has no level order): one workgroup per row
// b * n_gates + g, lanes on consecutive words.  Wire w of instance b is row b * n_in + w of the input block for w < n_in, else row
// b * n_outs + (w - n_in) of the block of gate outputs behind it; the term list, the coefficients, the constant and the source rows depend on
// blockIdx.x alone (wave-uniform).  The same arithmetic in the same order: canonical on read, canonical products and sums, the constant in
// the body only.  SNAP as in lwe_combine_kernel.
template <bool SNAP>
__global__ void __launch_bounds__(256) lwe_combine_rows_kernel(CombineRowsArgs a) {
    const size_t b = blockIdx.x / a.n_gates;
    const unsigned g = blockIdx.x % a.n_gates;
    const u64 t0 = a.first[g], t1 = a.first[g + 1];
    const u64 c = a.cst[g];
    u64* out = a.out + (size_t)blockIdx.x * a.words;
    const unsigned sl = SNAP ? a.slots[g] : 0;
    for (unsigned j = threadIdx.x; j < a.words; j += 256) {
        u64 s = j + 1 == a.words ? c : 0;
        for (u64 t = t0; t < t1; ++t) {
            const u32 w = a.src[t];
            const size_t row = w < a.n_in ? b * a.n_in + w : a.instances * a.n_in + b * a.n_outs + (w - a.n_in);
            s = gl::add(s, gl::mul(a.coef[t], gl::canon(a.wires[row * a.words + j])));
        }
        out[j] = SNAP ? multi_lut::snap(s, a.log_n, sl) : s;
    }
}

// dst row i = src row map[i] (map null: row i), rows of `words` words: the per-gate test vectors of a chunk, and the outputs put back into the
// caller's gate order.  One workgroup per row.
__global__ void __launch_bounds__(256) gather_rows_kernel(const u64* __restrict__ src, const u32* __restrict__ map, size_t words,
                                                          u64* __restrict__ dst) {
    const u64* s = src + (size_t)(map ? map[blockIdx.x] : blockIdx.x) * words;
    u64* d = dst + (size_t)blockIdx.x * words;
    for (size_t j = threadIdx.x; j < words; j += 256) d[j] = s[j];
}

struct Csr {   // a description in one gate order
    std::vector<u64> first, coef, cst;
    std::vector<u32> src, lut;
};
struct DeviceCsr {
    u64 *first = nullptr, *coef = nullptr, *cst = nullptr;
    u32 *src = nullptr, *lut = nullptr;
};
}  // namespace
}  // namespace vpbs

struct vpbs_program {
    vpbs_ctx* ctx = nullptr;   // null: host-only
    unsigned n_inputs = 0, n_gates = 0, n_luts = 0, n_levels = 0;
    size_t n_terms = 0;
    vpbs::Csr given;                   // the caller's order (host copy: prove gathers test vectors by it)
    std::vector<unsigned> level;       // [n_gates], caller's order
    std::vector<u32> order;            // permuted position q -> caller's gate
    std::vector<u32> level_first;      // [n_levels + 1] in permuted positions
    vpbs::DeviceCsr d_given, d_perm;   // d_perm.src: rows of the permuted wire table
    u32 *d_wire_pos = nullptr, *d_gate_pos = nullptr;   // caller's wire / gate -> row of the permuted wire table / permuted position
    u32* d_term_loc = nullptr;         // [n_terms][3], permuted term order: where a batched evaluation finds the term's source (run_batch)
    // multi-output gates (vpbs_program_create_multi): gate g has outs[g] output wires n_inputs + out_first[g] + j, its input is snapped by
    // slots[g].  multi is false for a description in which every gate is (0, 1): such a program IS one made by vpbs_program_create.
    bool multi = false;
    unsigned n_outs = 0;               // sum of outs: n_gates when !multi
    std::vector<u32> slots, out_first; // [n_gates], [n_gates + 1], caller's order
    std::vector<u32> pout_first;       // [n_gates + 1]: prefix sums of outs in permuted order (rows of the permuted wire table behind the inputs)
    u32 *d_given_slots = nullptr, *d_perm_slots = nullptr;   // multi only
    u32 *d_given_ext = nullptr, *d_perm_ext = nullptr;       // multi only: index [n_outs] | src gate [n_outs] of every output row, both orders
    std::vector<void*> owned;

    ~vpbs_program() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
    }
    template <class T>
    T* upload(const std::vector<T>& v) {
        T* d = static_cast<T*>(ctx->alloc_bytes(std::max<size_t>(8, v.size() * sizeof(T))));
        owned.push_back(d);
        if (!v.empty()) VPBS_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return d;
    }
    vpbs::DeviceCsr upload(const vpbs::Csr& c) {
        vpbs::DeviceCsr d;
        d.first = upload(c.first);
        d.coef = upload(c.coef);
        d.cst = upload(c.cst);
        d.src = upload(c.src);
        d.lut = upload(c.lut);
        return d;
    }
};

namespace vpbs {
namespace {
void launch_combine(hipStream_t s, const u64* d_wires, const DeviceCsr& d, unsigned gate0, unsigned count, unsigned words, u64* d_out,
                    const u32* d_slots = nullptr, unsigned log_n = 0) {
    const CombineArgs a{d_wires, d.first, d.src, d.coef, d.cst, d_out, gate0, words, d_slots, log_n};
    if (d_slots) hipLaunchKernelGGL(lwe_combine_kernel<true>, dim3(count), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(lwe_combine_kernel<false>, dim3(count), dim3(256), 0, s, a);
}
// a gate's slots against the ring of the object that evaluates or verifies it: false, with the message that names the gate
bool slots_fit(const vpbs_program* prog, unsigned log_n, std::string* msg) {
    for (unsigned g = 0; g < prog->n_gates && prog->multi; ++g)
        if (prog->slots[g] > log_n) {
            *msg = "gate " + std::to_string(g) + ": 2^gate_log_slots = 2^" + std::to_string(prog->slots[g]) + " exceeds N = " +
                   std::to_string((size_t)1 << log_n);
            return false;
        }
    return true;
}
// the shape refusal of verify / verify_batch, for a shape that arrives as numbers: N a power of two, 1 <= n_lwe <= (K - 1) N
bool extraction_shape(unsigned N, unsigned K, unsigned n_lwe, unsigned* log_n) {
    unsigned l = 0;
    while (l < 16 && (1u << l) < N) ++l;
    *log_n = l;
    return N != 0 && (1u << l) == N && K >= 2 && K <= (1u << 20) / N && n_lwe != 0 && n_lwe <= (size_t)(K - 1) * N;
}

// The gate inputs a verifier recomputes, on the host, word for word what verify / verify_batch leave in d_cts: per instance the wire table is
// the inputs followed by the extraction at coefficient j of every claimed output (multi_lut::extract_at_word; j = 0 is lwe_extract_kernel's
// row), then lwe_combine_kernel's arithmetic per gate -- canonical on read, canonical products and sums, the constant in the body word only
// -- and, for a program with multi-output gates, the snap of the gate's log_slots.  The shape has been checked (extraction_shape, slots_fit).
void gate_inputs_host(const vpbs_program* prog, unsigned log_n, unsigned K, unsigned n_lwe, const u64* inputs, size_t instances, const u64* out_cts,
                      u64* cts_out) {
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates;
    const size_t n = (size_t)1 << log_n, kn = K * n, words = (size_t)n_lwe + 1;
    const Csr& G = prog->given;
    std::vector<u64> wires(((size_t)n_in + prog->n_outs) * words);
    for (size_t b = 0; b < instances; ++b) {
        if (n_in) std::memcpy(wires.data(), inputs + b * n_in * words, 8 * n_in * words);
        for (unsigned g = 0; g < n_gates; ++g) {
            const u64* ct = out_cts + (b * n_gates + g) * kn;
            for (u32 o = prog->out_first[g]; o < prog->out_first[g + 1]; ++o) {
                u64* row = wires.data() + ((size_t)n_in + o) * words;
                for (unsigned c = 0; c <= n_lwe; ++c) row[c] = multi_lut::extract_at_word(ct, log_n, K, n_lwe, o - prog->out_first[g], c);
            }
        }
        for (unsigned g = 0; g < n_gates; ++g) {
            u64* out = cts_out + (b * n_gates + g) * words;
            for (size_t j = 0; j < words; ++j) {
                u64 s = j + 1 == words ? G.cst[g] : 0;
                for (u64 t = G.first[g]; t < G.first[g + 1]; ++t) s = gl::add(s, gl::mul(G.coef[t], gl::canon(wires[(size_t)G.src[t] * words + j])));
                out[j] = prog->multi ? multi_lut::snap(s, log_n, prog->slots[g]) : s;
            }
        }
    }
}

// what the three host statement functions refuse of (prog, N, K, n_lwe): false with the message, `who` in front
bool statement_shape_ok(const vpbs_program* prog, unsigned N, unsigned K, unsigned n_lwe, const std::string& who, unsigned* log_n, std::string* msg) {
    if (!prog) return *msg = who + ": null program", false;
    if (!extraction_shape(N, K, n_lwe, log_n))
        return *msg = who + ": the shape has no sample extraction (N a power of two, 1 <= n_lwe <= (K - 1) N)", false;
    std::string fit;
    if (!slots_fit(prog, *log_n, &fit)) return *msg = who + ": " + fit, false;
    return true;
}

void launch_gather(hipStream_t s, const u64* d_src, const u32* d_map, size_t words, unsigned rows, u64* d_dst) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(rows), dim3(256), 0, s, d_src, d_map, words, d_dst);
}

// device memory of one call, from a context's pool; released after the stream has drained
struct Scratch {
    vpbs_ctx* ctx;
    std::vector<void*> blocks;
    explicit Scratch(vpbs_ctx* c) : ctx(c) {}
    u64* words(size_t n) {
        u64* d = ctx->alloc_words(std::max<size_t>(1, n));
        blocks.push_back(d);
        return d;
    }
    ~Scratch() {
        if (blocks.empty()) return;
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : blocks) ctx->release(p);
    }
};

// vpbs_program_run; `b`'s runs are serialised by the caller
long program_run(vpbs_program* prog, vpbs_bootstrapper* b, const u64* inputs, const u64* testvs, u64* wires_out, u64* gate_cts_out, u64* out_cts,
                 int on_device) {
    if (!prog || !b || !prog->ctx) return VPBS_ERR_INVALID;
    BootstrapperShape sh{};
    bootstrapper_shape(b, &sh);
    vpbs_ctx* ctx = sh.ctx;
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = (size_t)1 << sh.prm.log_N, kn = sh.prm.K * n, n_wires = (size_t)n_in + prog->n_outs;
    const bool multi = prog->multi;
    const std::vector<u32>& pof = prog->pout_first;
    if (ctx->device != prog->ctx->device) return ctx->err = "the program and the Bootstrapper are on different devices", VPBS_ERR_INVALID;
    if ((n_in && !inputs) || (n_gates && !testvs)) return ctx->err = "null inputs or testvs", VPBS_ERR_INVALID;
    {
        std::string msg;
        if (!slots_fit(prog, sh.prm.log_N, &msg)) return ctx->err = msg, VPBS_ERR_INVALID;
    }
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            // the wire table in permuted order: inputs, then the gates level by level
            u64* d_wires = mem.words(n_wires * words);
            u64* d_cts = mem.words((size_t)n_gates * words);
            u64* d_out = out_cts || multi ? mem.words((size_t)n_gates * kn) : nullptr;   // multi: the wires are extracted from it
            const size_t chunk_max = std::min<size_t>(sh.max_batch, std::max(1u, n_gates));
            u64* d_tv = mem.words(chunk_max * n);
            const u64* d_testvs = testvs;
            if (on_device) {
                if (n_in) VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * (size_t)n_in * words, hipMemcpyDeviceToDevice, s));
            } else {
                if (n_in) VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * (size_t)n_in * words, hipMemcpyHostToDevice, s));
                if (n_gates) {
                    u64* d = mem.words((size_t)prog->n_luts * n);
                    VPBS_HIP(hipMemcpyAsync(d, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
                    d_testvs = d;
                }
            }
            for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
                for (size_t q0 = prog->level_first[lv]; q0 < prog->level_first[lv + 1]; q0 += sh.max_batch) {
                    const unsigned c = (unsigned)std::min<size_t>(sh.max_batch, prog->level_first[lv + 1] - q0);
                    {
                        vpbs::Timed t(ctx, "lwe_combine");
                        launch_combine(s, d_wires, prog->d_perm, (unsigned)q0, c, words, d_cts + q0 * words, multi ? prog->d_perm_slots : nullptr,
                                       sh.prm.log_N);
                    }
                    launch_gather(s, d_testvs, prog->d_perm.lut + q0, n, c, d_tv);
                    VPBS_HIP(hipGetLastError());
                    if (!multi) {
                        bootstrapper_enqueue(b, d_cts + q0 * words, c, d_tv, 1, d_out ? d_out + q0 * kn : nullptr,
                                             d_wires + ((size_t)n_in + q0) * words, nullptr);
                        continue;
                    }
                    // out_ct only; the chunk's output rows (contiguous in the permuted table) are extracted from it behind the launch
                    bootstrapper_enqueue(b, d_cts + q0 * words, c, d_tv, 1, d_out + q0 * kn, nullptr, nullptr);
                    vpbs::Timed t(ctx, "lwe_extract_at");
                    lwe_extract_at_enqueue(s, d_out, prog->d_perm_ext + pof[q0], prog->d_perm_ext + prog->n_outs + pof[q0], sh.prm.log_N, sh.prm.K,
                                           sh.n_lwe, pof[q0 + c] - pof[q0], d_wires + ((size_t)n_in + pof[q0]) * words);
                }
            }
            // back into the caller's order, to where the caller wants it
            auto deliver = [&](u64* dst, const u64* d_src, const u32* d_map, size_t row_words, size_t rows) {
                if (!dst || rows == 0) return;
                u64* d_dst = on_device ? dst : mem.words(rows * row_words);
                launch_gather(s, d_src, d_map, row_words, (unsigned)rows, d_dst);
                VPBS_HIP(hipGetLastError());
                if (!on_device) VPBS_HIP(hipMemcpyAsync(dst, d_dst, 8 * rows * row_words, hipMemcpyDeviceToHost, s));
            };
            deliver(wires_out, d_wires, prog->d_wire_pos, words, n_wires);
            deliver(gate_cts_out, d_cts, prog->d_gate_pos, words, n_gates);
            deliver(out_cts, out_cts ? d_out : nullptr, prog->d_gate_pos, kn, n_gates);
            VPBS_HIP(vpbs::stream_sync(s));   // the one wait
        } catch (const DeviceError&) {
            (void)vpbs::stream_sync(s);
            throw;
        }
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : (e.status == VPBS_ERR_INVALID ? VPBS_ERR_INVALID : VPBS_ERR_DEVICE);
    }
    return rc == VPBS_OK ? (long)prog->n_levels : rc;
}
// vpbs_program_run_batch
long program_run_batch(vpbs_program* prog, vpbs_keyring* ring, const u64* inputs, size_t instances, const u32* key_of, const u64* testvs,
                       u64* wires_out, u64* gate_cts_out, u64* out_cts, int on_device) {
    if (!ring) {   // no ring, no mutex: the message goes to the program's context alone
        if (prog && prog->ctx) prog->ctx->err = "vpbs_program_run_batch: null ring";
        return VPBS_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lock(keyring_mutex(ring));   // from the checks to the one wait: add, remove and run of the ring wait
    KeyringShape sh{};
    keyring_shape(ring, &sh);
    vpbs_ctx* ctx = sh.ctx;
    auto refuse = [&](const std::string& m) {   // under the ring's mutex, as every writer of its context's message
        ctx->err = m;
        return (long)VPBS_ERR_INVALID;
    };
    if (!prog) return refuse("vpbs_program_run_batch: null program");
    if (!prog->ctx) return refuse("vpbs_program_run_batch: a host-only program (made without a context) cannot be evaluated");
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = (size_t)1 << sh.prm.log_N, kn = sh.prm.K * n, n_outs = prog->n_outs, n_wires = (size_t)n_in + n_outs, B = instances;
    const bool multi = prog->multi;
    const std::vector<u32>& pof = prog->pout_first;
    if (ctx->device != prog->ctx->device) return refuse("vpbs_program_run_batch: the program and the ring are on different devices");
    {
        std::string fit;
        if (!slots_fit(prog, sh.prm.log_N, &fit)) return refuse("vpbs_program_run_batch: " + fit);
    }
    if (B && ((n_in && !inputs) || (n_gates && !testvs) || !key_of)) return refuse("vpbs_program_run_batch: null inputs, testvs or key_of");
    if (n_wires && B > 0x7fffffffull / n_wires) return refuse("vpbs_program_run_batch: instances x wires exceeds 2^31 - 1 rows");
    std::string msg;
    if (!keyring_check_slots(ring, key_of, B, "vpbs_program_run_batch", "instance", &msg)) return refuse(msg);
    if (B == 0) return (long)prog->n_levels;
    if (n_gates == 0) {   // the wires are the inputs: nothing to launch, no index to build
        if (!wires_out || !n_in) return 0;
        if (!on_device) return std::memcpy(wires_out, inputs, 8 * B * n_in * words), 0;
        try {
            VPBS_HIP(hipSetDevice(ctx->device));
            VPBS_HIP(hipMemcpyAsync(wires_out, inputs, 8 * B * n_in * words, hipMemcpyDeviceToDevice, ctx->stream));
            VPBS_HIP(vpbs::stream_sync(ctx->stream));
        } catch (const DeviceError& e) {
            ctx->err = e.what;
            return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
        }
        return 0;
    }
    const std::vector<u32>& lf = prog->level_first;
    // ---- the instances in slot order (stable), and every index array of every launch ----
    std::vector<u32> inst(B), pos_of(B), gate_pos(n_gates);
    {
        std::vector<size_t> start(sh.max_keys + 1, 0);
        for (size_t b = 0; b < B; ++b) ++start[key_of[b] + 1];
        for (size_t k = 0; k < sh.max_keys; ++k) start[k + 1] += start[k];
        for (size_t b = 0; b < B; ++b) {
            pos_of[b] = (u32)start[key_of[b]]++;
            inst[pos_of[b]] = (u32)b;
        }
    }
    for (unsigned q = 0; q < n_gates; ++q) gate_pos[prog->order[q]] = q;
    size_t widest = 0;
    for (unsigned lv = 0; lv < prog->n_levels; ++lv) widest = std::max<size_t>(widest, lf[lv + 1] - lf[lv]);
    const size_t chunk_max = std::max<size_t>(1, std::min<size_t>(sh.max_batch, B * widest)), rows_g = B * n_gates, rows_w = B * n_wires;
    const bool want_gates = gate_cts_out || out_cts;
    // identity [chunk_max] | key_of of every gate row | gate_lut of every gate row | input rows | caller's wire rows | caller's gate rows
    // multi: | extraction index of every output row | its gate row -- both in the order of the level-major block of outputs
    const size_t o_key = chunk_max, o_lut = o_key + rows_g, o_in = o_lut + rows_g, o_wire = o_in + B * n_in,
                 o_gate = o_wire + (wires_out ? rows_w : 0), o_ext = o_gate + (want_gates ? rows_g : 0), total = o_ext + (multi ? 2 * B * n_outs : 0);
    std::vector<u32> idx(total);   // lives until the wait
    // row of output 0 of gate-row r (instance position r / w, gate lf[lv] + r % w) of level lv among the output rows of the level-major
    // table; r = B * w gives the end of the level's block
    auto out_row = [&](unsigned lv, size_t r) {
        const size_t w = lf[lv + 1] - lf[lv];
        return B * pof[lf[lv]] + (r / w) * (pof[lf[lv + 1]] - pof[lf[lv]]) + (pof[lf[lv] + r % w] - pof[lf[lv]]);
    };
    if (multi)
        for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
            const size_t w = lf[lv + 1] - lf[lv];
            for (size_t r = 0; r < B * w; ++r) {
                const size_t o = out_row(lv, r), m = pof[lf[lv] + r % w + 1] - pof[lf[lv] + r % w];
                for (size_t j = 0; j < m; ++j) {
                    idx[o_ext + o + j] = (u32)j;
                    idx[o_ext + B * n_outs + o + j] = (u32)(B * lf[lv] + r);
                }
            }
        }
    for (size_t i = 0; i < chunk_max; ++i) idx[i] = (u32)i;
    for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
        const size_t w = lf[lv + 1] - lf[lv], base = B * lf[lv];
        for (size_t s = 0; s < B; ++s)
            for (size_t j = 0; j < w; ++j) {
                idx[o_key + base + s * w + j] = key_of[inst[s]];
                idx[o_lut + base + s * w + j] = prog->given.lut[prog->order[lf[lv] + j]];
            }
    }
    for (size_t s = 0; s < B; ++s)
        for (unsigned w = 0; w < n_in; ++w) idx[o_in + s * n_in + w] = (u32)((size_t)inst[s] * n_in + w);
    auto gate_row = [&](size_t b, unsigned g) {   // row of gate g of instance b among the gate rows of the level-major table
        const unsigned lv = prog->level[g] - 1;
        return B * lf[lv] + (size_t)pos_of[b] * (lf[lv + 1] - lf[lv]) + (gate_pos[g] - lf[lv]);
    };
    for (size_t b = 0; b < B; ++b) {
        if (wires_out) {
            for (unsigned w = 0; w < n_in; ++w) idx[o_wire + b * n_wires + w] = (u32)((size_t)pos_of[b] * n_in + w);
            for (unsigned g = 0; g < n_gates && !multi; ++g) idx[o_wire + b * n_wires + n_in + g] = (u32)(B * n_in + gate_row(b, g));
            for (unsigned g = 0; g < n_gates && multi; ++g) {   // the gate's outputs lie side by side in its level's block of outputs
                const unsigned lv = prog->level[g] - 1;
                const size_t o = out_row(lv, (size_t)pos_of[b] * (lf[lv + 1] - lf[lv]) + (gate_pos[g] - lf[lv]));
                for (u32 j = prog->out_first[g]; j < prog->out_first[g + 1]; ++j)
                    idx[o_wire + b * n_wires + n_in + j] = (u32)(B * n_in + o + (j - prog->out_first[g]));
            }
        }
        if (want_gates)
            for (unsigned g = 0; g < n_gates; ++g) idx[o_gate + b * n_gates + g] = (u32)gate_row(b, g);
    }
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            u32* d_idx = reinterpret_cast<u32*>(mem.words((total + 1) / 2));
            VPBS_HIP(hipMemcpyAsync(d_idx, idx.data(), sizeof(u32) * total, hipMemcpyHostToDevice, s));   // once, before the first launch
            u64* d_wires = mem.words(rows_w * words);
            u64* d_cts = mem.words(rows_g * words);
            u64* d_out = out_cts || multi ? mem.words(rows_g * kn) : nullptr;   // multi: the wires are extracted from it
            u64* d_tv = mem.words(chunk_max * n);
            const u64 *d_testvs = testvs, *d_inputs = inputs;
            if (!on_device) {
                u64* d = mem.words((size_t)prog->n_luts * n);
                VPBS_HIP(hipMemcpyAsync(d, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
                d_testvs = d;
                if (n_in) {
                    d = mem.words(B * n_in * words);
                    VPBS_HIP(hipMemcpyAsync(d, inputs, 8 * B * n_in * words, hipMemcpyHostToDevice, s));
                    d_inputs = d;
                }
            }
            if (n_in) {   // the block of inputs, the instances in slot order, as given
                launch_gather(s, d_inputs, d_idx + o_in, words, (unsigned)(B * n_in), d_wires);
                VPBS_HIP(hipGetLastError());
            }
            for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
                const size_t w = lf[lv + 1] - lf[lv], rows = B * w, base = B * lf[lv];
                for (size_t r0 = 0; r0 < rows; r0 += sh.max_batch) {
                    const unsigned c = (unsigned)std::min<size_t>(sh.max_batch, rows - r0);
                    u64* cts = d_cts + (base + r0) * words;
                    {
                        vpbs::Timed t(ctx, "lwe_combine");
                        const CombineBatchArgs a{d_wires, prog->d_perm.first, prog->d_term_loc, prog->d_perm.coef, prog->d_perm.cst, cts, B,
                                                 (unsigned)r0, lf[lv], (unsigned)w, words, multi ? prog->d_perm_slots : nullptr, sh.prm.log_N};
                        if (multi) hipLaunchKernelGGL(lwe_combine_batch_kernel<true>, dim3(c), dim3(256), 0, s, a);
                        else hipLaunchKernelGGL(lwe_combine_batch_kernel<false>, dim3(c), dim3(256), 0, s, a);
                    }
                    launch_gather(s, d_testvs, d_idx + o_lut + base + r0, n, c, d_tv);
                    VPBS_HIP(hipGetLastError());
                    // the rows are in slot order already: the identity as `order`, the rows' own slots as `key_of`
                    if (!multi) {
                        keyring_enqueue(ring, cts, c, d_tv, 1, d_idx, d_idx + o_key + base + r0, d_out ? d_out + (base + r0) * kn : nullptr,
                                        d_wires + (B * n_in + base + r0) * words, nullptr);
                        continue;
                    }
                    // out_ct only; the chunk's output rows are a contiguous piece of the level's block of outputs
                    keyring_enqueue(ring, cts, c, d_tv, 1, d_idx, d_idx + o_key + base + r0, d_out + (base + r0) * kn, nullptr, nullptr);
                    const size_t o0 = out_row(lv, r0), o1 = out_row(lv, r0 + c);
                    vpbs::Timed t(ctx, "lwe_extract_at");
                    lwe_extract_at_enqueue(s, d_out, d_idx + o_ext + o0, d_idx + o_ext + B * n_outs + o0, sh.prm.log_N, sh.prm.K, sh.n_lwe, o1 - o0,
                                           d_wires + (B * n_in + o0) * words);
                }
            }
            // back into the caller's instance and gate order, to where the caller wants it
            auto deliver = [&](u64* dst, const u64* d_src, const u32* d_map, size_t row_words, size_t rows) {
                if (!dst || rows == 0) return;
                u64* d_dst = on_device ? dst : mem.words(rows * row_words);
                {
                    vpbs::Timed t(ctx, "program_deliver");
                    launch_gather(s, d_src, d_map, row_words, (unsigned)rows, d_dst);
                }
                VPBS_HIP(hipGetLastError());
                if (!on_device) VPBS_HIP(hipMemcpyAsync(dst, d_dst, 8 * rows * row_words, hipMemcpyDeviceToHost, s));
            };
            deliver(wires_out, d_wires, d_idx + o_wire, words, rows_w);
            deliver(gate_cts_out, d_cts, d_idx + o_gate, words, rows_g);
            deliver(out_cts, out_cts ? d_out : nullptr, d_idx + o_gate, kn, rows_g);
            VPBS_HIP(vpbs::stream_sync(s));   // the one wait
        } catch (const DeviceError&) {
            (void)vpbs::stream_sync(s);
            throw;
        }
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : (e.status == VPBS_ERR_INVALID ? VPBS_ERR_INVALID : VPBS_ERR_DEVICE);
    }
    return rc == VPBS_OK ? (long)prog->n_levels : rc;
}
// vpbs_program_create (slots_in, outs_in null: every gate (0, 1)) and vpbs_program_create_multi
int program_create(vpbs_ctx* ctx, const vpbs_program_desc* desc, const unsigned* slots_in, const unsigned* outs_in, vpbs_program** out, char* err,
                   size_t err_len) {
    if (out) *out = nullptr;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        if (ctx) ctx->err = m;
        return VPBS_ERR_INVALID;
    };
    if (!desc || !out) return refuse("null argument");
    const unsigned n_in = desc->n_inputs, n_gates = desc->n_gates;
    const size_t T = desc->n_terms;
    if (n_gates && (!desc->gate_first || !desc->gate_const || !desc->gate_lut)) return refuse("null argument");
    if (T && (!desc->term_src || !desc->term_coef || !n_gates)) return refuse("null argument");
    if ((u64)n_in + n_gates > 0x7fffffffull) return refuse("too many wires");
    const bool described = slots_in || outs_in;
    if (described && n_gates && (!slots_in || !outs_in)) return refuse("null argument");
    // ---- validity, gate by gate ----
    if (n_gates && desc->gate_first[0] != 0) return refuse("gate 0: gate_first does not start at 0");
    std::vector<u32> out_first(n_gates + 1, 0);   // output j of gate g is wire n_inputs + out_first[g] + j
    bool multi = false;
    for (unsigned g = 0; g < n_gates; ++g) {
        const std::string gate = "gate " + std::to_string(g) + ": ";
        const unsigned sl = described ? slots_in[g] : 0, m = described ? outs_in[g] : 1;
        if (sl > 16) return refuse(gate + "gate_log_slots " + std::to_string(sl) + " exceeds 16");
        if (m == 0) return refuse(gate + "gate_outputs is 0");
        if (m > (1u << sl)) return refuse(gate + "gate_outputs " + std::to_string(m) + " exceeds 2^gate_log_slots = " + std::to_string(1u << sl));
        if ((u64)n_in + out_first[g] + m > 0x7fffffffull) return refuse(gate + "too many wires");
        out_first[g + 1] = out_first[g] + m;
        multi = multi || sl != 0 || m != 1;
        const u64 t0 = desc->gate_first[g], t1 = desc->gate_first[g + 1];
        if (t1 < t0 || t1 > T) return refuse(gate + "gate_first is not monotone within [0, n_terms]");
        if (desc->gate_lut[g] >= desc->n_luts) return refuse(gate + "gate_lut " + std::to_string(desc->gate_lut[g]) + " is not below n_luts");
        if (desc->gate_const[g] >= gl::P) return refuse(gate + "gate_const is not below p");
        for (u64 t = t0; t < t1; ++t) {
            if (desc->term_src[t] >= (u64)n_in + out_first[g])   // out_first[g] = g when every gate has one output
                return refuse(gate + "term " + std::to_string(t - t0) + " reads wire " + std::to_string(desc->term_src[t]) +
                              ", which is not below n_inputs + " + std::to_string(out_first[g]) + " (topological order)");
            if (desc->term_coef[t] >= gl::P) return refuse(gate + "term " + std::to_string(t - t0) + ": term_coef is not below p");
        }
    }
    if (n_gates && desc->gate_first[n_gates] != T)
        return refuse("gate " + std::to_string(n_gates - 1) + ": gate_first ends at " + std::to_string(desc->gate_first[n_gates]) + ", not at n_terms");
    // ---- levels, and the order that makes them contiguous (stable: the caller's order within a level) ----
    auto* p = new vpbs_program;
    p->n_inputs = n_in;
    p->n_gates = n_gates;
    p->n_luts = desc->n_luts;
    p->n_terms = T;
    Csr& G = p->given;
    G.first.assign(desc->gate_first, desc->gate_first + (n_gates ? n_gates + 1 : 0));
    if (!n_gates) G.first.assign(1, 0);
    G.src.assign(desc->term_src, desc->term_src + T);
    G.coef.assign(desc->term_coef, desc->term_coef + T);
    G.cst.assign(desc->gate_const, desc->gate_const + n_gates);
    G.lut.assign(desc->gate_lut, desc->gate_lut + n_gates);
    const unsigned n_outs = out_first[n_gates];
    p->multi = multi;
    p->n_outs = n_outs;
    p->out_first = out_first;
    p->slots.assign(n_gates, 0);
    if (described) std::copy(slots_in, slots_in + n_gates, p->slots.begin());
    std::vector<u32> gate_of(n_outs);   // output wire - n_inputs -> its gate
    for (unsigned g = 0; g < n_gates; ++g) std::fill(gate_of.begin() + out_first[g], gate_of.begin() + out_first[g + 1], g);
    p->level.resize(n_gates);
    for (unsigned g = 0; g < n_gates; ++g) {
        unsigned lv = 0;
        for (u64 t = G.first[g]; t < G.first[g + 1]; ++t)
            if (G.src[t] >= n_in) lv = std::max(lv, p->level[gate_of[G.src[t] - n_in]]);
        p->level[g] = lv + 1;
        p->n_levels = std::max(p->n_levels, lv + 1);
    }
    p->level_first.assign(p->n_levels + 1, 0);
    for (unsigned g = 0; g < n_gates; ++g) ++p->level_first[p->level[g]];
    for (unsigned lv = 0; lv < p->n_levels; ++lv) p->level_first[lv + 1] += p->level_first[lv];
    p->order.resize(n_gates);
    std::vector<u32> gate_pos(n_gates), wire_pos((size_t)n_in + n_outs);
    {
        std::vector<u32> next(p->level_first.begin(), p->level_first.end());
        for (unsigned g = 0; g < n_gates; ++g) {
            const u32 q = next[p->level[g] - 1]++;
            p->order[q] = g;
            gate_pos[g] = q;
        }
    }
    // the permuted wire table: inputs, then the OUTPUTS of the gates level by level (a gate's outputs side by side)
    std::vector<u32>& pof = p->pout_first;
    pof.assign(n_gates + 1, 0);
    for (unsigned q = 0; q < n_gates; ++q) pof[q + 1] = pof[q] + (out_first[p->order[q] + 1] - out_first[p->order[q]]);
    for (unsigned w = 0; w < n_in; ++w) wire_pos[w] = w;
    for (unsigned g = 0; g < n_gates; ++g)
        for (u32 j = out_first[g]; j < out_first[g + 1]; ++j) wire_pos[n_in + j] = n_in + pof[gate_pos[g]] + (j - out_first[g]);
    if (ctx) {
        Csr R;   // the permuted description; sources are rows of the permuted wire table
        std::vector<u32> term_loc;   // per term of R: the source's block in a level-major table (first row per instance, width, position)
        R.first.push_back(0);
        for (unsigned q = 0; q < n_gates; ++q) {
            const unsigned g = p->order[q];
            for (u64 t = G.first[g]; t < G.first[g + 1]; ++t) {
                const u32 row = wire_pos[G.src[t]];
                R.src.push_back(row);
                R.coef.push_back(G.coef[t]);
                if (row < n_in) {
                    term_loc.insert(term_loc.end(), {0u, n_in, row});
                } else {
                    const unsigned lv = p->level[gate_of[G.src[t] - n_in]] - 1;
                    const u32 o0 = pof[p->level_first[lv]], o1 = pof[p->level_first[lv + 1]];   // the level's block of outputs
                    term_loc.insert(term_loc.end(), {n_in + o0, o1 - o0, row - n_in - o0});
                }
            }
            R.first.push_back(R.src.size());
            R.cst.push_back(G.cst[g]);
            R.lut.push_back(G.lut[g]);
        }
        p->ctx = ctx;
        try {
            VPBS_HIP(hipSetDevice(ctx->device));
            p->d_given = p->upload(G);
            p->d_perm = p->upload(R);
            p->d_wire_pos = p->upload(wire_pos);
            p->d_gate_pos = p->upload(gate_pos);
            p->d_term_loc = p->upload(term_loc);
            if (multi) {
                std::vector<u32> perm_slots(n_gates), given_ext(2 * (size_t)n_outs), perm_ext(2 * (size_t)n_outs);
                for (unsigned q = 0; q < n_gates; ++q) {
                    const unsigned g = p->order[q];
                    perm_slots[q] = p->slots[g];
                    for (u32 j = 0; j < out_first[g + 1] - out_first[g]; ++j) {
                        given_ext[out_first[g] + j] = perm_ext[pof[q] + j] = j;
                        given_ext[n_outs + out_first[g] + j] = g;
                        perm_ext[n_outs + pof[q] + j] = q;
                    }
                }
                p->d_given_slots = p->upload(p->slots);
                p->d_perm_slots = p->upload(perm_slots);
                p->d_given_ext = p->upload(given_ext);
                p->d_perm_ext = p->upload(perm_ext);
            }
            VPBS_HIP(vpbs::stream_sync(ctx->stream));   // the staging vectors go away
        } catch (const DeviceError& e) {
            (void)vpbs::stream_sync(ctx->stream);
            report(err, err_len, e.what);
            ctx->err = e.what;
            delete p;
            return e.status;
        }
    }
    *out = p;
    report(err, err_len, "");
    return VPBS_OK;
}
}  // namespace
}  // namespace vpbs

extern "C" {
int vpbs_program_create(vpbs_ctx* ctx, const vpbs_program_desc* desc, vpbs_program** out, char* err, size_t err_len) {
    return vpbs::program_create(ctx, desc, nullptr, nullptr, out, err, err_len);
}

int vpbs_program_create_multi(vpbs_ctx* ctx, const vpbs_program_desc* desc, const unsigned* gate_log_slots, const unsigned* gate_outputs,
                              vpbs_program** out, char* err, size_t err_len) {
    if (desc && desc->n_gates && (!gate_log_slots || !gate_outputs)) {
        if (out) *out = nullptr;
        vpbs::report(err, err_len, "null argument");
        if (ctx) ctx->err = "null argument";
        return VPBS_ERR_INVALID;
    }
    static const unsigned none = 0;   // a program without gates: the arrays may be null
    return vpbs::program_create(ctx, desc, gate_log_slots ? gate_log_slots : &none, gate_outputs ? gate_outputs : &none, out, err, err_len);
}

void vpbs_program_free(vpbs_program* prog) { delete prog; }

long vpbs_program_wires(const vpbs_program* prog, unsigned* out_first_out) {
    if (!prog) return VPBS_ERR_INVALID;
    if (out_first_out) std::copy(prog->out_first.begin(), prog->out_first.end(), out_first_out);
    return (long)prog->n_inputs + (long)prog->n_outs;
}

long vpbs_program_levels(const vpbs_program* prog, unsigned* levels_out) {
    if (!prog) return VPBS_ERR_INVALID;
    if (levels_out) std::copy(prog->level.begin(), prog->level.end(), levels_out);
    return (long)prog->n_levels;
}

long vpbs_program_run(vpbs_program* prog, vpbs_bootstrapper* bootstrapper, const uint64_t* inputs, const uint64_t* testvs, uint64_t* wires_out,
                      uint64_t* gate_cts_out, uint64_t* out_cts, int on_device) {
    return vpbs::program_run(prog, bootstrapper, inputs, testvs, wires_out, gate_cts_out, out_cts, on_device);
}

long vpbs_program_run_batch(vpbs_program* prog, vpbs_keyring* ring, const uint64_t* inputs, size_t instances, const uint32_t* key_of,
                            const uint64_t* testvs, uint64_t* wires_out, uint64_t* gate_cts_out, uint64_t* out_cts, int on_device) {
    return vpbs::program_run_batch(prog, ring, inputs, instances, key_of, testvs, wires_out, gate_cts_out, out_cts, on_device);
}

long vpbs_program_prove(vpbs_program* prog, vpbs_pbs_prover* pbs_prover, const uint64_t* inputs, const uint64_t* testvs, unsigned steps,
                        uint64_t* wires_out, uint64_t* out_cts, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    using namespace vpbs;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!prog || !pbs_prover) return refuse("null program or prover");
    if (!prog->ctx) return refuse("a host-only program (made without a context) cannot be evaluated");
    if (!proof_fn) return refuse("no proof_fn: the proofs have nowhere to go");
    if ((prog->n_inputs && !inputs) || (prog->n_gates && !testvs)) return refuse("null inputs or testvs");
    std::mutex* boot_mu = nullptr;
    vpbs_bootstrapper* boot = pbs_prover_bootstrapper(pbs_prover, &boot_mu);
    BootstrapperShape sh{};
    bootstrapper_shape(boot, &sh);
    if (steps > sh.n_lwe + 2) return refuse("steps exceeds n_lwe + 2 = " + std::to_string(sh.n_lwe + 2));
    const size_t n = (size_t)1 << sh.prm.log_N, words = sh.n_lwe + 1;
    std::vector<u64> gate_cts((size_t)prog->n_gates * words), tv((size_t)prog->n_gates * n);
    {
        std::lock_guard<std::mutex> lk(*boot_mu);
        const long rc = program_run(prog, boot, inputs, testvs, wires_out, gate_cts.data(), out_cts, 0);
        if (rc < 0) return report(err, err_len, std::string("evaluating the program: ") + vpbs_last_error(sh.ctx)), rc;
    }
    if (prog->n_gates == 0) return 0;
    for (unsigned g = 0; g < prog->n_gates; ++g) std::memcpy(tv.data() + (size_t)g * n, testvs + (size_t)prog->given.lut[g] * n, 8 * n);
    return vpbs_pbs_prover_run(pbs_prover, gate_cts.data(), prog->n_gates, tv.data(), 1, steps, nullptr, nullptr, proof_fn, user, err, err_len);
}

long vpbs_program_prove_batch(vpbs_program* prog, vpbs_ring_prover* ring_prover, const uint64_t* inputs, size_t instances, const uint32_t* key_of,
                              const uint64_t* testvs, unsigned steps, uint64_t* wires_out, uint64_t* out_cts, vpbs_pbs_proof_fn proof_fn, void* user,
                              char* err, size_t err_len) {
    using namespace vpbs;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!ring_prover) return refuse("vpbs_program_prove_batch: null ring prover");
    if (!prog) return refuse("vpbs_program_prove_batch: null program");
    if (!proof_fn) return refuse("no proof_fn: the proofs have nowhere to go");
    vpbs_keyring* ring = vpbs_ring_prover_keyring(ring_prover);
    KeyringShape sh{};
    keyring_shape(ring, &sh);
    if (steps > sh.n_lwe + 2) return refuse("steps exceeds n_lwe + 2 = " + std::to_string(sh.n_lwe + 2));
    const size_t n = (size_t)1 << sh.prm.log_N, words = sh.n_lwe + 1, n_gates = prog->n_gates;
    // from the evaluation to the last proof no key set comes or goes: the ring takes them from its prover alone, and the prover waits here
    std::lock_guard<std::mutex> run(ring_prover_mutex(ring_prover));
    if (n_gates && instances > 0x7fffffffull / n_gates) return refuse("vpbs_program_prove_batch: instances x gates exceeds 2^31 - 1 rows");
    std::vector<u64> gate_cts(instances * n_gates * words);
    // the refusals are run_batch's: checked there before anything is queued, the message in the ring's context
    const long rc = program_run_batch(prog, ring, inputs, instances, key_of, testvs, wires_out, gate_cts.empty() ? nullptr : gate_cts.data(), out_cts, 0);
    if (rc < 0) return report(err, err_len, std::string("evaluating the program: ") + vpbs_last_error(sh.ctx)), rc;
    if (n_gates == 0 || instances == 0) return 0;
    // row b * n_gates + g: gate g of instance b, with the gate's test vector and the instance's slot
    std::vector<u64> tv(instances * n_gates * n);
    std::vector<u32> slot_of(instances * n_gates);
    for (size_t b = 0; b < instances; ++b)
        for (size_t g = 0; g < n_gates; ++g) {
            std::memcpy(tv.data() + (b * n_gates + g) * n, testvs + (size_t)prog->given.lut[g] * n, 8 * n);
            slot_of[b * n_gates + g] = key_of[b];
        }
    return ring_prover_run_locked(ring_prover, gate_cts.data(), instances * n_gates, slot_of.data(), tv.data(), 1, steps, nullptr, nullptr, proof_fn,
                                  user, err, err_len);
}

long vpbs_program_verify(vpbs_program* prog, vpbs_pbs_verifier* pbs_verifier, const uint64_t* inputs, const uint64_t* testvs,
                         const uint64_t* out_cts, const uint8_t* proofs, const size_t* offsets, uint8_t* verdicts, uint8_t* reasons,
                         uint8_t* proof_reasons) {
    using namespace vpbs;
    if (!prog || !pbs_verifier || !prog->ctx || !offsets || !verdicts) return VPBS_ERR_INVALID;
    PbsVerifierShape sh{};
    pbs_verifier_shape(pbs_verifier, &sh);
    vpbs_ctx* ctx = sh.ctx;
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = sh.N, kn = (size_t)sh.K * n;
    if (ctx->device != prog->ctx->device) return ctx->err = "the program and the verifier are on different devices", VPBS_ERR_INVALID;
    if (n_gates == 0) return 0;
    if ((n_in && !inputs) || !testvs || !out_cts || !proofs) return ctx->err = "null inputs, testvs, out_cts or proofs", VPBS_ERR_INVALID;
    unsigned log_n = 0;
    while (((size_t)1 << log_n) < n) ++log_n;
    if (((size_t)1 << log_n) != n || sh.K < 2 || sh.n_lwe == 0 || sh.n_lwe > (sh.K - 1) * n)
        return ctx->err = "the verifier's shape has no sample extraction (N a power of two, 1 <= n_lwe <= (K - 1) N)", VPBS_ERR_INVALID;
    {
        std::string msg;
        if (!slots_fit(prog, log_n, &msg)) return ctx->err = msg, VPBS_ERR_INVALID;
    }
    const bool multi = prog->multi;
    const size_t n_outs = prog->n_outs;
    std::vector<u64> cts((size_t)n_gates * words), tv((size_t)n_gates * n);
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            u64* d_wires = mem.words(((size_t)n_in + n_outs) * words);   // the caller's order: inputs, then the extractions
            u64* d_out = mem.words((size_t)n_gates * kn);
            u64* d_cts = mem.words((size_t)n_gates * words);
            if (n_in) VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * (size_t)n_in * words, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_out, out_cts, 8 * (size_t)n_gates * kn, hipMemcpyHostToDevice, s));
            if (!multi) lwe_extract_enqueue(s, d_out, log_n, sh.K, sh.n_lwe, n_gates, d_wires + (size_t)n_in * words);
            else   // every (gate, j) row in one launch
                lwe_extract_at_enqueue(s, d_out, prog->d_given_ext, prog->d_given_ext + n_outs, log_n, sh.K, sh.n_lwe, n_outs,
                                       d_wires + (size_t)n_in * words);
            {
                vpbs::Timed t(ctx, "lwe_combine");   // all gates at once: no level order
                launch_combine(s, d_wires, prog->d_given, 0, n_gates, words, d_cts, multi ? prog->d_given_slots : nullptr, log_n);
            }
            VPBS_HIP(hipGetLastError());
            VPBS_HIP(hipMemcpyAsync(cts.data(), d_cts, 8 * cts.size(), hipMemcpyDeviceToHost, s));
            VPBS_HIP(vpbs::stream_sync(s));
        } catch (const DeviceError&) {
            (void)vpbs::stream_sync(s);
            throw;
        }
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
    for (unsigned g = 0; g < n_gates; ++g) std::memcpy(tv.data() + (size_t)g * n, testvs + (size_t)prog->given.lut[g] * n, 8 * n);
    long accepted = 0;
    for (size_t g0 = 0; g0 < n_gates; g0 += sh.max_batch) {
        const size_t c = std::min<size_t>(sh.max_batch, n_gates - g0);
        const long rc = vpbs_pbs_verifier_run(pbs_verifier, proofs, offsets + g0, c, tv.data() + g0 * n, 1, cts.data() + g0 * words, out_cts + g0 * kn,
                                              verdicts + g0, reasons ? reasons + g0 : nullptr, proof_reasons ? proof_reasons + g0 : nullptr);
        if (rc < 0) return rc;
        accepted += rc;
    }
    return accepted;
}

long vpbs_program_verify_batch(vpbs_program* prog, vpbs_ring_verifier* ring_verifier, const uint64_t* inputs, size_t instances, const uint32_t* key_of,
                               const uint64_t* testvs, const uint64_t* out_cts, const uint8_t* proofs, const size_t* offsets, uint8_t* verdicts,
                               uint8_t* reasons, uint8_t* proof_reasons, char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_verify_batch";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!ring_verifier) return refuse(who + ": null ring verifier");
    if (!prog) return refuse(who + ": null program");
    if (!prog->ctx) return refuse(who + ": a host-only program (made without a context) cannot be verified");
    std::lock_guard<std::mutex> lock(ring_verifier_mutex(ring_verifier));   // from the check of the slots to the last wait
    RingVerifierShape sh{};
    ring_verifier_shape(ring_verifier, &sh);
    vpbs_ctx* ctx = sh.ctx;
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = sh.N, kn = (size_t)sh.K * n, n_outs = prog->n_outs, n_wires = (size_t)n_in + n_outs, B = instances, rows = B * n_gates;
    const bool multi = prog->multi;
    if (ctx->device != prog->ctx->device) return refuse(who + ": the program and the ring verifier are on different devices");
    if (n_wires && B > 0x7fffffffull / n_wires) return refuse(who + ": instances x wires exceeds 2^31 - 1 rows");
    if (B && !key_of) return refuse(who + ": null key_of");
    if (rows && ((n_in && !inputs) || !testvs || !out_cts || !proofs || !offsets || !verdicts))
        return refuse(who + ": null inputs, testvs, out_cts, proofs, offsets or verdicts");
    unsigned log_n = 0;
    while (((size_t)1 << log_n) < n) ++log_n;
    if (((size_t)1 << log_n) != n || sh.K < 2 || sh.n_lwe == 0 || sh.n_lwe > (sh.K - 1) * n)
        return refuse(who + ": the verifier's shape has no sample extraction (N a power of two, 1 <= n_lwe <= (K - 1) N)");
    std::string msg;
    if (!slots_fit(prog, log_n, &msg)) return refuse(who + ": " + msg);
    if (!ring_verifier_check_slots(ring_verifier, key_of, B, who.c_str(), "instance", &msg)) return refuse(msg);
    for (size_t r = 0; r < rows; ++r)
        if (offsets[r + 1] < offsets[r]) return refuse(who + ": offsets decrease at row " + std::to_string(r));
    if (rows == 0) return 0;
    // testv_of | key_of of every row, uploaded once; multi: | extraction index | claimed GLWE of every output row b * n_outs + o
    const size_t o_ext = 2 * rows, total = o_ext + (multi ? 2 * B * n_outs : 0);
    std::vector<u32> idx(total);   // lives until the last wait
    for (size_t b = 0; b < B; ++b)
        for (size_t g = 0; g < n_gates; ++g) {
            idx[b * n_gates + g] = prog->given.lut[g];
            idx[rows + b * n_gates + g] = key_of[b];
            for (u32 o = prog->out_first[g]; multi && o < prog->out_first[g + 1]; ++o) {
                idx[o_ext + b * n_outs + o] = o - prog->out_first[g];
                idx[o_ext + B * n_outs + b * n_outs + o] = (u32)(b * n_gates + g);
            }
        }
    PbsVerifyCore* core = ring_verifier_core(ring_verifier);
    long accepted = 0;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            u64* d_wires = mem.words(B * n_wires * words);   // [B][n_in] inputs, then [B][n_outs] extractions
            u64* d_out = mem.words(rows * kn);
            u64* d_cts = mem.words(rows * words);
            u64* d_testvs = mem.words((size_t)prog->n_luts * n);
            u32* d_idx = reinterpret_cast<u32*>(mem.words((total + 1) / 2));
            if (n_in) VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * B * n_in * words, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_out, out_cts, 8 * rows * kn, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_testvs, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_idx, idx.data(), sizeof(u32) * total, hipMemcpyHostToDevice, s));
            if (!multi) lwe_extract_enqueue(s, d_out, log_n, sh.K, sh.n_lwe, rows, d_wires + B * n_in * words);
            else
                lwe_extract_at_enqueue(s, d_out, d_idx + o_ext, d_idx + o_ext + B * n_outs, log_n, sh.K, sh.n_lwe, B * n_outs,
                                       d_wires + B * n_in * words);
            {
                vpbs::Timed t(ctx, "lwe_combine");
                const CombineRowsArgs a{d_wires, prog->d_given.first, prog->d_given.src, prog->d_given.coef, prog->d_given.cst, d_cts, B, n_in, n_gates,
                                        words, (unsigned)n_outs, multi ? prog->d_given_slots : nullptr, log_n};
                if (multi) hipLaunchKernelGGL(lwe_combine_rows_kernel<true>, dim3((unsigned)rows), dim3(256), 0, s, a);
                else hipLaunchKernelGGL(lwe_combine_rows_kernel<false>, dim3((unsigned)rows), dim3(256), 0, s, a);
            }
            VPBS_HIP(hipGetLastError());
            for (size_t r0 = 0; r0 < rows; r0 += sh.max_batch) {   // a chunk may straddle instances: every row brings its own indices
                const size_t c = std::min<size_t>(sh.max_batch, rows - r0);
                const int rc = pbs_verify_enqueue(core, proofs, offsets + r0, c, d_cts + r0 * words, d_out + r0 * kn, d_testvs, d_idx + r0,
                                                  ring_verifier_key_table(ring_verifier), d_idx + rows + r0);
                if (rc) {
                    (void)vpbs::stream_sync(s);
                    return report(err, err_len, who + ": malformed offsets"), (long)rc;
                }
                accepted += pbs_verify_collect(core, c, verdicts + r0, reasons ? reasons + r0 : nullptr, proof_reasons ? proof_reasons + r0 : nullptr);
            }
        } catch (const DeviceError& e) {
            pbs_verify_abandon(core, e);
            (void)vpbs::stream_sync(s);
            throw;
        }
    } catch (const DeviceError& e) {
        report(err, err_len, who + ": " + e.what);
        return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
    return accepted;
}

// ---- one proof per program instance ----
int vpbs_program_gate_inputs(const vpbs_program* prog, unsigned N, unsigned K, unsigned n_lwe, const uint64_t* inputs, size_t instances,
                             const uint64_t* out_cts, uint64_t* cts_out, char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_gate_inputs";
    report(err, err_len, "");
    unsigned log_n = 0;
    std::string msg;
    if (!statement_shape_ok(prog, N, K, n_lwe, who, &log_n, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    if (instances && prog->n_gates && ((prog->n_inputs && !inputs) || !out_cts || !cts_out))
        return report(err, err_len, who + ": null inputs, out_cts or cts_out"), VPBS_ERR_INVALID;
    gate_inputs_host(prog, log_n, K, n_lwe, inputs, instances, out_cts, cts_out);
    return VPBS_OK;
}

int vpbs_program_aggregate_root(const vpbs_program* prog, unsigned N, unsigned K, unsigned n_lwe, const uint64_t* vk0, const uint64_t* inputs,
                                const uint64_t* testvs, const uint64_t* out_cts, const uint64_t* key_hash, uint64_t out[4], char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_aggregate_root";
    report(err, err_len, "");
    unsigned log_n = 0;
    std::string msg;
    if (!statement_shape_ok(prog, N, K, n_lwe, who, &log_n, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    if (prog->n_gates == 0) return report(err, err_len, who + ": the program has no gates: there is nothing to aggregate"), VPBS_ERR_INVALID;
    if (!vk0 || (prog->n_inputs && !inputs) || !testvs || !out_cts || !key_hash || !out)
        return report(err, err_len, who + ": null vk0, inputs, testvs, out_cts, key_hash or out"), VPBS_ERR_INVALID;
    std::vector<u64> cts((size_t)prog->n_gates * (n_lwe + 1));
    gate_inputs_host(prog, log_n, K, n_lwe, inputs, 1, out_cts, cts.data());
    const int rc = vpbs_aggregate_root(N, K, n_lwe, vk0, prog->n_gates, testvs, prog->n_luts, prog->given.lut.data(), cts.data(), out_cts, key_hash, 1,
                                       nullptr, out);
    if (rc < 0) report(err, err_len, who + ": vpbs_aggregate_root refused the statement");
    return rc;
}

int vpbs_program_verify_aggregate(const vpbs_program* prog, const vpbs_aggregate_shape* shape, const uint64_t* inputs, const uint64_t* testvs,
                                  const uint64_t* out_cts, const uint64_t* key_hash, const uint8_t* bytes, size_t len, int* reason, char* why,
                                  size_t why_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_verify_aggregate";
    report(why, why_len, "");
    if (reason) *reason = VPBS_AGG_MALFORMED;
    if (!shape) return report(why, why_len, who + ": null shape"), VPBS_ERR_INVALID;
    unsigned log_n = 0;
    std::string msg;
    if (!statement_shape_ok(prog, shape->N, shape->K, shape->n_lwe, who, &log_n, &msg)) return report(why, why_len, msg), VPBS_ERR_INVALID;
    if (prog->n_gates == 0) return report(why, why_len, who + ": the program has no gates: there is nothing to aggregate"), VPBS_ERR_INVALID;
    if (shape->levels < 32 && prog->n_gates > ((size_t)1 << shape->levels))
        return report(why, why_len, who + ": n_gates " + std::to_string(prog->n_gates) + " exceeds 2^levels = " +
                                        std::to_string((size_t)1 << shape->levels)), VPBS_ERR_INVALID;
    if ((prog->n_inputs && !inputs) || !testvs || !out_cts || !key_hash || !bytes)
        return report(why, why_len, who + ": null inputs, testvs, out_cts, key_hash or bytes"), VPBS_ERR_INVALID;
    std::vector<u64> cts((size_t)prog->n_gates * (shape->n_lwe + 1));
    gate_inputs_host(prog, log_n, shape->K, shape->n_lwe, inputs, 1, out_cts, cts.data());
    return vpbs_verify_aggregate(shape, prog->n_gates, testvs, prog->n_luts, prog->given.lut.data(), cts.data(), out_cts, key_hash, 1, nullptr, bytes,
                                 len, reason, why, why_len);
}

}  // extern "C"

namespace {
// the proofs of a prove / prove_batch run, kept for the aggregator, and the caller's own proof_fn behind them
struct ProofSink {
    std::vector<std::vector<uint8_t>> proofs;
    std::vector<uint8_t> have;
    std::string failure;   // the first failing row, named
    vpbs_pbs_proof_fn fn;
    void* user;
    static void take(void* self, size_t index, const uint8_t* bytes, size_t len, const char* error) {
        auto* s = static_cast<ProofSink*>(self);
        if (index < s->proofs.size()) {
            if (bytes) {
                s->proofs[index].assign(bytes, bytes + len);
                s->have[index] = 1;
            } else if (s->failure.empty()) {
                s->failure = std::to_string(index) + ": " + (error ? error : "no proof");
            }
        }
        if (s->fn) s->fn(s->user, index, bytes, len, error);
    }
    // the proofs [first, first + count) in one buffer with offsets, as vpbs_aggregator_run takes them
    void pack(size_t first, size_t count, std::vector<uint8_t>* bytes, std::vector<size_t>* offsets) const {
        bytes->clear();
        offsets->assign(1, 0);
        for (size_t i = first; i < first + count; ++i) {
            bytes->insert(bytes->end(), proofs[i].begin(), proofs[i].end());
            offsets->push_back(bytes->size());
        }
    }
};
// the refusal both aggregate provers make before anything is proven: "" when the program fits the aggregator
std::string gates_fit(const vpbs_program* prog, const vpbs_aggregator* aggregator) {
    const unsigned levels = vpbs::aggregator_levels(aggregator);
    if (prog->n_gates == 0) return "the program has no gates: there is nothing to aggregate";
    if (prog->n_gates > ((size_t)1 << levels))
        return "n_gates " + std::to_string(prog->n_gates) + " exceeds 2^levels = " + std::to_string((size_t)1 << levels) + " of the aggregator";
    return "";
}
}  // namespace

extern "C" {
long vpbs_program_prove_aggregate(vpbs_program* prog, vpbs_pbs_prover* pbs_prover, vpbs_aggregator* aggregator, const uint64_t* inputs,
                                  const uint64_t* testvs, uint64_t* wires_out, uint64_t* out_cts, uint8_t* out, size_t capacity,
                                  vpbs_aggregate_stats* stats, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_prove_aggregate: ";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, who + m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (stats) *stats = vpbs_aggregate_stats{};
    if (!prog || !pbs_prover || !aggregator || !out) return refuse("null program, prover, aggregator or out");
    const std::string fit = gates_fit(prog, aggregator);
    if (!fit.empty()) return refuse(fit);
    ProofSink sink{std::vector<std::vector<uint8_t>>(prog->n_gates), std::vector<uint8_t>(prog->n_gates, 0), "", proof_fn, user};
    const long n = vpbs_program_prove(prog, pbs_prover, inputs, testvs, 0, wires_out, out_cts, &ProofSink::take, &sink, err, err_len);
    if (n < 0) return n;
    if (!sink.failure.empty() || (size_t)n != prog->n_gates) return refuse((sink.failure.empty() ? "proofs are missing" : "gate " + sink.failure) + "; nothing was aggregated");
    std::vector<uint8_t> bytes;
    std::vector<size_t> offsets;
    sink.pack(0, prog->n_gates, &bytes, &offsets);
    return vpbs_aggregator_run(aggregator, bytes.data(), offsets.data(), prog->n_gates, out, capacity, stats, err, err_len);
}

long vpbs_program_prove_aggregate_batch(vpbs_program* prog, vpbs_ring_prover* ring_prover, vpbs_aggregator* aggregator, const uint64_t* inputs,
                                        size_t instances, const uint32_t* key_of, const uint64_t* testvs, uint64_t* wires_out, uint64_t* out_cts,
                                        vpbs_aggregate_fn agg_fn, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_prove_aggregate_batch: ";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, who + m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!prog || !ring_prover || !aggregator) return refuse("null program, ring prover or aggregator");
    if (!agg_fn) return refuse("no agg_fn: the aggregates have nowhere to go");
    const std::string fit = gates_fit(prog, aggregator);
    if (!fit.empty()) return refuse(fit);
    const size_t G = prog->n_gates;
    if (instances > 0x7fffffffull / G) return refuse("instances x gates exceeds 2^31 - 1 rows");
    ProofSink sink{std::vector<std::vector<uint8_t>>(instances * G), std::vector<uint8_t>(instances * G, 0), "", proof_fn, user};
    const long n = vpbs_program_prove_batch(prog, ring_prover, inputs, instances, key_of, testvs, 0, wires_out, out_cts, &ProofSink::take, &sink, err,
                                            err_len);
    if (n < 0) return n;
    if (!sink.failure.empty() || (size_t)n != instances * G)
        return refuse((sink.failure.empty() ? "proofs are missing" : "row " + sink.failure + " (row b * n_gates + g)") + "; nothing was aggregated");
    std::vector<uint8_t> bytes, agg(aggregator_max_bytes(aggregator));
    std::vector<size_t> offsets;
    if (aggregator_device_witness(aggregator) && instances) {   // ONE run: the level-l nodes of all instances in the same device batches
        sink.pack(0, instances * G, &bytes, &offsets);
        const std::vector<size_t> counts(instances, G);
        struct Hand {
            vpbs_aggregate_fn fn;
            void* user;
        } hand{agg_fn, user};
        const long done = vpbs_aggregator_run_many(aggregator, bytes.data(), offsets.data(), counts.data(), instances,
                                                   [](void* h, size_t tree, const uint8_t* proof, size_t len) {
                                                       auto* x = static_cast<Hand*>(h);
                                                       x->fn(tree, proof, len, x->user);
                                                   }, &hand, err, err_len);
        return done < 0 ? done : (long)instances;
    }
    for (size_t b = 0; b < instances; ++b) {
        sink.pack(b * G, G, &bytes, &offsets);
        const long len = vpbs_aggregator_run(aggregator, bytes.data(), offsets.data(), G, agg.data(), agg.size(), nullptr, err, err_len);
        if (len < 0) return len;
        agg_fn(b, agg.data(), (size_t)len, user);
    }
    return (long)instances;
}

long vpbs_program_verify_aggregate_batch(vpbs_program* prog, vpbs_aggregate_verifier* agg_verifier, const uint64_t* inputs, size_t instances,
                                         const uint32_t* key_of, const uint64_t* key_hashes, size_t n_keys, const uint64_t* testvs,
                                         const uint64_t* out_cts, const uint8_t* bytes, const size_t* offsets, uint8_t* verdicts, uint8_t* reasons,
                                         char* err, size_t err_len) {
    using namespace vpbs;
    const std::string who = "vpbs_program_verify_aggregate_batch";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!agg_verifier) return refuse(who + ": null aggregate verifier");
    if (!prog) return refuse(who + ": null program");
    if (!prog->ctx) return refuse(who + ": a host-only program (made without a context) cannot be verified on the device");
    AggregateVerifierShape sh{};
    aggregate_verifier_shape(agg_verifier, &sh);
    vpbs_ctx* ctx = sh.ctx;
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = sh.N, kn = (size_t)sh.K * n, n_outs = prog->n_outs, n_wires = (size_t)n_in + n_outs, B = instances, rows = B * n_gates;
    const bool multi = prog->multi;
    if (ctx->device != prog->ctx->device) return refuse(who + ": the program and the aggregate verifier are on different devices");
    unsigned log_n = 0;
    std::string msg;
    if (!statement_shape_ok(prog, sh.N, sh.K, sh.n_lwe, who, &log_n, &msg)) return refuse(msg);
    if (n_gates == 0) return refuse(who + ": the program has no gates: there is nothing to aggregate");
    if (n_gates > ((size_t)1 << sh.levels) || n_gates > sh.max_leaves)
        return refuse(who + ": n_gates " + std::to_string(n_gates) + " exceeds 2^levels = " + std::to_string((size_t)1 << sh.levels) +
                      " or max_leaves " + std::to_string(sh.max_leaves) + " of the aggregate verifier");
    if (n_wires && B > 0x7fffffffull / n_wires) return refuse(who + ": instances x wires exceeds 2^31 - 1 rows");
    if (B && (!key_of || !key_hashes || (n_in && !inputs) || !testvs || !out_cts || !bytes || !offsets || !verdicts))
        return refuse(who + ": null key_of, key_hashes, inputs, testvs, out_cts, bytes, offsets or verdicts");
    for (size_t b = 0; b < B; ++b) {
        if (key_of[b] >= n_keys)
            return refuse(who + ": key_of[" + std::to_string(b) + "] = " + std::to_string(key_of[b]) + " is not below n_keys " + std::to_string(n_keys));
        if (offsets[b + 1] < offsets[b]) return refuse(who + ": offsets decrease at instance " + std::to_string(b));
    }
    if (B == 0) return 0;
    // instances per run of the verifier; testv_of = gate_lut tiled, key_of of the row's instance, the trees' first leaves: host arrays
    const size_t per = std::min(sh.max_aggregates, sh.max_leaves / n_gates);
    std::vector<u32> lut_of(per * n_gates), key_row(rows);
    std::vector<size_t> leaf_first(per + 1);
    for (size_t b = 0; b < per; ++b) std::copy(prog->given.lut.begin(), prog->given.lut.end(), lut_of.begin() + b * n_gates);
    for (size_t b = 0; b <= per; ++b) leaf_first[b] = b * n_gates;
    for (size_t b = 0; b < B; ++b) std::fill(key_row.begin() + b * n_gates, key_row.begin() + (b + 1) * n_gates, key_of[b]);
    std::vector<u32> ext;   // multi: extraction index | claimed GLWE of every output row b * n_outs + o (as verify_batch)
    if (multi) {
        ext.resize(2 * B * n_outs);
        for (size_t b = 0; b < B; ++b)
            for (size_t g = 0; g < n_gates; ++g)
                for (u32 o = prog->out_first[g]; o < prog->out_first[g + 1]; ++o) {
                    ext[b * n_outs + o] = o - prog->out_first[g];
                    ext[B * n_outs + b * n_outs + o] = (u32)(b * n_gates + g);
                }
    }
    long accepted = 0;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            u64* d_wires = mem.words(B * n_wires * words);   // [B][n_in] inputs, then [B][n_outs] extractions
            u64* d_out = mem.words(rows * kn);
            u64* d_cts = mem.words(rows * words);
            u64* d_testvs = mem.words((size_t)prog->n_luts * n);
            u64* d_khs = mem.words(4 * n_keys);
            u32* d_ext = multi ? reinterpret_cast<u32*>(mem.words(B * n_outs)) : nullptr;
            if (n_in) VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * B * n_in * words, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_out, out_cts, 8 * rows * kn, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_testvs, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_khs, key_hashes, 32 * n_keys, hipMemcpyHostToDevice, s));
            if (multi) VPBS_HIP(hipMemcpyAsync(d_ext, ext.data(), sizeof(u32) * ext.size(), hipMemcpyHostToDevice, s));
            if (!multi) lwe_extract_enqueue(s, d_out, log_n, sh.K, sh.n_lwe, rows, d_wires + B * n_in * words);
            else lwe_extract_at_enqueue(s, d_out, d_ext, d_ext + B * n_outs, log_n, sh.K, sh.n_lwe, B * n_outs, d_wires + B * n_in * words);
            {
                vpbs::Timed t(ctx, "lwe_combine");
                const CombineRowsArgs a{d_wires, prog->d_given.first, prog->d_given.src, prog->d_given.coef, prog->d_given.cst, d_cts, B, n_in, n_gates,
                                        words, (unsigned)n_outs, multi ? prog->d_given_slots : nullptr, log_n};
                if (multi) hipLaunchKernelGGL(lwe_combine_rows_kernel<true>, dim3((unsigned)rows), dim3(256), 0, s, a);
                else hipLaunchKernelGGL(lwe_combine_rows_kernel<false>, dim3((unsigned)rows), dim3(256), 0, s, a);
            }
            VPBS_HIP(hipGetLastError());
            // the verifier's stages follow on the same stream: the tables stay where they are
            for (size_t b0 = 0; b0 < B; b0 += per) {
                const size_t c = std::min(per, B - b0), r0 = b0 * n_gates;
                const long rc = vpbs_aggregate_verifier_run_many(agg_verifier, bytes, offsets + b0, c, leaf_first.data(), d_testvs, prog->n_luts,
                                                                 lut_of.data(), d_cts + r0 * words, d_out + r0 * kn, d_khs, n_keys, key_row.data() + r0, 1,
                                                                 verdicts + b0, reasons ? reasons + b0 : nullptr, err, err_len);
                if (rc < 0) return rc;
                accepted += rc;
            }
        } catch (const DeviceError&) {
            (void)vpbs::stream_sync(s);
            throw;
        }
    } catch (const DeviceError& e) {
        report(err, err_len, who + ": " + e.what);
        return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
    return accepted;
}
}  // extern "C"

// Programs of lookup gates on resident keys (vpbs_program, include/vpbs_prover.h): a netlist whose every gate is one bootstrap of a linear
// combination of earlier wires.  The object validates and levelises the description on the host and keeps it twice: in the caller's gate
// order (a verifier combines all gates at once) and permuted level by level (an evaluation walks the levels).
//
// ONE combination.  combine_word is one output word of one gate, for host and device: the constant in the body word, plus
// coef * canon(source word) per term, then the snap of a multi-output program.  A term finds its source row of a LEVEL-MAJOR wire table
// -- the block of inputs [instances][n_inputs], then blocks [instances][width] of gate outputs -- through a triple (first, width, pos):
// row = instances * first + inst * width + pos.  Both orders carry such triples (program_create): the permuted description has one block
// per level, the caller's order ONE block of all outputs, so its table is [instances][n_inputs] | [instances][n_outs].  The device runs
// the word in lwe_combine_batch_kernel, one workgroup per (instance, gate) row; gate_inputs_host runs it in a loop over the same triples.
// The single-key evaluation reads the row of its one instance directly (RowSource, the kernel's ONE instantiation).
//
// ONE evaluation (program_walk).  Per level, per chunk of max_batch rows of the level's block, on the context's stream:
//             lwe_combine_batch_kernel   wire table -> the chunk's gate inputs  [rows][n_lwe + 1]
//             gather_rows_kernel         testvs[gate_lut of the row] -> the chunk's test vectors  [rows][N]
//             the bootstrap launch       -> out_ct, and lwe_out straight into the level's block (contiguous rows)
//           then gather_rows_kernel delivers wires, gate inputs and output GLWEs in the caller's order, and the host waits once.  The
//           levels are ordered by the stream; nothing waits inside a kernel for another workgroup.
//   run        one instance on a Bootstrapper (vpbs::bootstrapper_enqueue): the inputs are copied straight into the table, and every index
//           table is the program's own, resident since create -- with one instance the level-major table IS the permuted wire table.
//   run_batch  `instances` input sets, instance b under the key set of slot key_of[b] of a key ring (vpbs::keyring_enqueue).  The instances
//           stand in slot order (a stable sort of key_of on the host), so that a chunk of consecutive rows is grouped by key set; every
//           index array of every launch is uploaded once, before the first launch.
//   prove   run on the batch prover's Bootstrapper, then vpbs_pbs_prover_run on the gate inputs (caller's order) with per-gate test vectors.
//   prove_batch  run_batch on the ring of a ring prover (pbs_prove_ring.hip), then vpbs_ring_prover_run on the gate inputs of every instance,
//           row b * n_gates + g under the slot of instance b, under the prover's mutex from the evaluation to the last proof.
//
// ONE statement on the device (statement_enqueue), for every verifier: upload inputs, claimed outputs and test vectors of all instances, ONE
// extraction launch on all outputs, ONE combine launch over all rows (instance, gate) in the caller's order.
//   verify, verify_batch  the statement, then the rows where they lie to the verifier's core (verify_rows: vpbs::pbs_verify_enqueue on device
//           pointers per chunk of max_batch rows, one wait per chunk for the result bytes) -- the test vector of a row through
//           testv_of = gate_lut, the key hash through key_of of the row's instance.  verify is one instance on a PbsVerifier's core and
//           one-entry key table; verify_batch is all instances on a ring verifier (verify_pbs_batch.hip), under its mutex.
//   One proof per program instance: the gates of an instance are the leaves of ONE aggregate (aggregate.hip), in gate order.
//   gate_inputs, aggregate_root, verify_aggregate   the statement on the HOST (a host-only program will do): the wire table from the claimed
//           outputs (multi_lut::extract_at_word), combine_word per gate, then vpbs_aggregate_root / vpbs_verify_aggregate over those gate
//           inputs with testv_of = gate_lut.
//   prove_aggregate, prove_aggregate_batch   prove / prove_batch with the proofs kept, then vpbs_aggregator_run per instance, after the last proof.
//   verify_aggregate_batch   the statement, then the tables where they lie to vpbs_aggregate_verifier_run_many (device pointers;
//           testv_of = gate_lut tiled, the key index per row), in chunks of the verifier's max_aggregates / max_leaves on the same stream,
//           one wait per chunk.
//
// Multi-output gates (vpbs_program_create_multi): gate g has outs[g] output wires and a snap of slots[g].  Everything above
// holds with "outputs of the level" for "gates of the level" in the wire tables; the gate inputs, the output GLWEs and the proofs stay
// per gate.  For such a program (multi): the combine kernel runs in its SNAP instantiation, the bootstrap launch writes out_ct only,
// and ONE lwe_extract_at_kernel launch per chunk (multi_lut.hip) fills the chunk's output rows -- contiguous in the table -- behind it on
// the same stream; the statement extracts all (gate, j) rows in one launch.  A description whose every gate is (0, 1) is not multi: it
// runs exactly the launches listed above.
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
// A description in one gate order, as host or as device pointers.
struct CombineTable {
    const u64 *first, *coef, *cst;   // [n_gates + 1], [n_terms], [n_gates]
    const u32* loc;                  // [n_terms][3]: the source of a term in a level-major wire table -- the block's first row per instance,
                                     // the block's width, the position in the block
    const u32* slots;                // SNAP only, [n_gates]: log2 of the gate's slots (multi_lut.h)
    const u32* src;                  // the permuted order on the device only, [n_terms]: the source's row of ONE instance's table (RowSource)
};
// Where term t finds its source row: by the triple, for any number of instances ...
struct BlockSource {
    const u32* loc;
    size_t instances, inst;
    GL_HD size_t operator()(u64 t) const {
        const u32* l = loc + 3 * t;
        return instances * l[0] + inst * l[1] + l[2];
    }
};
// ... and the same row as ONE load where there is one instance: the single-key evaluation queues a combine launch of a few rows per chunk
// of every level, and its event time is 12 % longer with the triple's three loads (profiles/program_one_body.json).
struct RowSource {
    const u32* src;
    GL_HD size_t operator()(u64 t) const { return src[t]; }
};

// Word j of a gate's input.  A wire word is reduced before it is used (an input ciphertext may hold words at or above p; bootstrap outputs
// are canonical); products and sums are canonical in, canonical out; the constant goes into the body word only.  SNAP (programs with
// multi-output gates): the canonical sum is rounded by the gate's own slots_log; log_n is the ring's.  [t0, t1), cst and sl are the gate's
// entries of the table, read once per row by the caller.
template <bool SNAP, class Source>
GL_HD u64 combine_word(const u64* coef, u64 t0, u64 t1, u64 cst, unsigned sl, const u64* wires, const Source& row_of, size_t words, size_t j,
                       unsigned log_n) {
    u64 s = j + 1 == words ? cst : 0;
    for (u64 t = t0; t < t1; ++t) s = gl::add(s, gl::mul(coef[t], gl::canon(wires[row_of(t) * words + j])));
    return SNAP ? multi_lut::snap(s, log_n, sl) : s;
}

struct CombineArgs {
    const u64* wires;       // a level-major wire table
    CombineTable d;
    u64* out;               // [count][words]: row 0 is row `row0` of the block of rows [instances][width]
    size_t instances;
    unsigned row0, gate0, width, words;   // gate0: the first gate of the block; width: gates per instance in it; words = n_lwe + 1
    unsigned log_n;
};

// One workgroup per (instance, gate) row, lanes on consecutive words: row r of the block is gate gate0 + r % width of the instance at
// position r / width.  The term list, the coefficients, the constant and the source rows depend on blockIdx.x alone (wave-uniform), and a
// term is one coalesced read of a wire row.  An evaluation's block is a level (of the permuted description); a verifier's is all gates
// (gate0 = 0, row0 = 0, width = n_gates, the caller's order).  ONE: instances == 1 and d.src is there -- row r is gate gate0 + r.
template <bool SNAP, bool ONE>
__global__ void __launch_bounds__(256) lwe_combine_batch_kernel(CombineArgs a) {
    const unsigned r = a.row0 + blockIdx.x;
    const size_t inst = ONE ? 0 : r / a.width;
    const unsigned g = a.gate0 + (ONE ? r : r % a.width);
    const u64 t0 = a.d.first[g], t1 = a.d.first[g + 1];
    const u64 c = a.d.cst[g];
    u64* out = a.out + (size_t)blockIdx.x * a.words;
    const unsigned sl = SNAP ? a.d.slots[g] : 0;
    for (unsigned j = threadIdx.x; j < a.words; j += 256)
        out[j] = ONE ? combine_word<SNAP>(a.d.coef, t0, t1, c, sl, a.wires, RowSource{a.d.src}, a.words, j, a.log_n)
                     : combine_word<SNAP>(a.d.coef, t0, t1, c, sl, a.wires, BlockSource{a.d.loc, a.instances, inst}, a.words, j, a.log_n);
}

// dst row i = src row map[i] (map null: row i), rows of `words` words: the per-gate test vectors of a chunk, and the outputs put back into the
// caller's gate order.  One workgroup per row.
__global__ void __launch_bounds__(256) gather_rows_kernel(const u64* __restrict__ src, const u32* __restrict__ map, size_t words,
                                                          u64* __restrict__ dst) {
    const u64* s = src + (size_t)(map ? map[blockIdx.x] : blockIdx.x) * words;
    u64* d = dst + (size_t)blockIdx.x * words;
    for (size_t j = threadIdx.x; j < words; j += 256) d[j] = s[j];
}

struct Csr {   // a description in one gate order, on the host
    std::vector<u64> first, coef, cst;
    std::vector<u32> src, loc, lut, slots;   // src: the wire a term reads (the caller's order), its row of the permuted wire table (permuted)
    CombineTable table() const { return {first.data(), coef.data(), cst.data(), loc.data(), slots.data(), nullptr}; }   // for BlockSource
};
struct DeviceCsr {
    CombineTable d{};          // d.slots: multi only; d.src: the permuted order only
    u32* lut = nullptr;        // [n_gates]
    u32* ext = nullptr;        // multi only: index [n_outs] | source gate [n_outs] of every output row of one instance (lwe_extract_at_enqueue)
};
}  // namespace
}  // namespace vpbs

struct vpbs_program {
    vpbs_ctx* ctx = nullptr;   // null: host-only
    unsigned n_inputs = 0, n_gates = 0, n_luts = 0, n_levels = 0;
    size_t n_terms = 0;
    vpbs::Csr given;                   // the caller's order (lut: prove gathers test vectors by it; slots: all zero when !multi)
    std::vector<unsigned> level;       // [n_gates], caller's order
    std::vector<u32> order;            // permuted position q -> caller's gate
    std::vector<u32> level_first;      // [n_levels + 1] in permuted positions
    unsigned widest = 0;               // gates of the widest level
    vpbs::DeviceCsr d_given, d_perm;
    u32 *d_wire_pos = nullptr, *d_gate_pos = nullptr;   // caller's wire / gate -> row of the permuted wire table / permuted position
    // multi-output gates (vpbs_program_create_multi): gate g has outs[g] output wires n_inputs + out_first[g] + j, its input is snapped by
    // given.slots[g].  multi is false for a description in which every gate is (0, 1): such a program IS one made by vpbs_program_create.
    bool multi = false;
    unsigned n_outs = 0;               // sum of outs: n_gates when !multi
    std::vector<u32> out_first;        // [n_gates + 1], caller's order
    std::vector<u32> pout_first;       // [n_gates + 1]: prefix sums of outs in permuted order (rows of the permuted wire table behind the inputs)
    std::vector<void*> owned;

    // In the level-major table of B instances: the row of output 0 of gate row r (instance position r / w, gate level_first[lv] + r % w) of
    // level lv among the output rows; r = B * w gives the end of the level's block.
    size_t out_row(size_t B, unsigned lv, size_t r) const {
        const std::vector<u32>&pof = pout_first, &lf = level_first;
        const size_t w = lf[lv + 1] - lf[lv];
        return B * pof[lf[lv]] + (r / w) * (pof[lf[lv + 1]] - pof[lf[lv]]) + (pof[lf[lv] + r % w] - pof[lf[lv]]);
    }
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
    vpbs::DeviceCsr upload(const vpbs::Csr& c, const std::vector<u32>& ext, bool with_src) {
        vpbs::DeviceCsr d;
        d.d = {upload(c.first), upload(c.coef), upload(c.cst), upload(c.loc), multi ? upload(c.slots) : nullptr, with_src ? upload(c.src) : nullptr};
        d.lut = upload(c.lut);
        if (multi) d.ext = upload(ext);
        return d;
    }
};

namespace vpbs {
namespace {
// the one combine launch: `count` rows from row `row0` of the block [instances][width] whose first gate is gate0 of `d`
void combine_enqueue(vpbs_ctx* ctx, const vpbs_program* prog, const DeviceCsr& d, const u64* d_wires, size_t instances, unsigned row0, unsigned gate0,
                     unsigned width, unsigned count, unsigned words, unsigned log_n, u64* d_out) {
    vpbs::Timed t(ctx, "lwe_combine");
    const CombineArgs a{d_wires, d.d, d_out, instances, row0, gate0, width, words, log_n};
    const bool one = instances == 1 && d.d.src;   // one instance of the permuted order: the level-major table is the permuted wire table
    auto* kernel = prog->multi ? (one ? lwe_combine_batch_kernel<true, true> : lwe_combine_batch_kernel<true, false>)
                               : (one ? lwe_combine_batch_kernel<false, true> : lwe_combine_batch_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(count), dim3(256), 0, ctx->stream, a);
}
// a gate's slots against the ring of the object that evaluates or verifies it: false, with the message that names the gate
bool slots_fit(const vpbs_program* prog, unsigned log_n, std::string* msg) {
    for (unsigned g = 0; g < prog->n_gates && prog->multi; ++g)
        if (prog->given.slots[g] > log_n) {
            *msg = "gate " + std::to_string(g) + ": 2^gate_log_slots = 2^" + std::to_string(prog->given.slots[g]) + " exceeds N = " +
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

// The gate inputs a verifier recomputes, on the host, word for word what statement_enqueue leaves in d_cts: the wire table of all instances
// in the caller's order -- [instances][n_in] inputs, then [instances][n_outs] extractions at coefficient j of the claimed outputs
// (multi_lut::extract_at_word; j = 0 is lwe_extract_kernel's row) -- then combine_word per (instance, gate) row.  The shape has been checked
// (extraction_shape, slots_fit).
void gate_inputs_host(const vpbs_program* prog, unsigned log_n, unsigned K, unsigned n_lwe, const u64* inputs, size_t instances, const u64* out_cts,
                      u64* cts_out) {
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates;
    const size_t n = (size_t)1 << log_n, kn = K * n, words = (size_t)n_lwe + 1, n_outs = prog->n_outs, B = instances;
    const CombineTable d = prog->given.table();
    std::vector<u64> wires(B * (n_in + n_outs) * words);
    if (B * n_in) std::memcpy(wires.data(), inputs, 8 * B * n_in * words);
    for (size_t b = 0; b < B; ++b)
        for (unsigned g = 0; g < n_gates; ++g) {
            const u64* ct = out_cts + (b * n_gates + g) * kn;
            for (u32 o = prog->out_first[g]; o < prog->out_first[g + 1]; ++o) {
                u64* row = wires.data() + (B * n_in + b * n_outs + o) * words;
                for (unsigned c = 0; c <= n_lwe; ++c) row[c] = multi_lut::extract_at_word(ct, log_n, K, n_lwe, o - prog->out_first[g], c);
            }
        }
    for (size_t b = 0; b < B; ++b)
        for (unsigned g = 0; g < n_gates; ++g) {
            u64* out = cts_out + (b * n_gates + g) * words;
            const BlockSource row_of{d.loc, B, b};
            for (size_t j = 0; j < words; ++j)
                out[j] = prog->multi ? combine_word<true>(d.coef, d.first[g], d.first[g + 1], d.cst[g], d.slots[g], wires.data(), row_of, words, j, log_n)
                                     : combine_word<false>(d.coef, d.first[g], d.first[g + 1], d.cst[g], 0, wires.data(), row_of, words, j, log_n);
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

// what an evaluation needs of the object that bootstraps for it (a Bootstrapper, a key ring)
struct WalkShape {
    vpbs_ctx* ctx;
    vpbs_tfhe_params prm;
    unsigned n_lwe;
    size_t max_batch;
};
// The device index tables of one evaluation of B instances, over the level-major wire table and its gate rows (row B * level_first[lv] + r is
// row r of level lv's block [B][gates of the level]).
struct WalkTables {
    const u32* lut;        // [B n_gates]: the test vector of every gate row
    const u32* in_map;     // [B n_in]: the row of the inputs as given that goes to each row of the block of inputs; null: copied as given
    const u32* wire_map;   // [B n_wires]: the table row of every wire in the caller's (instance, wire) order
    const u32* gate_map;   // [B n_gates]: the gate row of every gate in the caller's (instance, gate) order
    const u32* ext;        // multi: extraction index [B n_outs] | source gate row [B n_outs] of every output row of the table
};

// The level walk of vpbs_program_run (B = 1) and vpbs_program_run_batch, after their checks.  tables(mem, stream) gives the WalkTables --
// resident ones, or the caller's one upload -- and bootstrap(d_cts, count, d_tv, row, d_out_ct, d_lwe_out) queues the ONE bootstrap launch
// of `count` <= max_batch rows from gate row `row`, with per-row test vectors.  -> the number of levels, or the status with the message in
// the context.
template <class Tables, class Bootstrap>
long program_walk(const vpbs_program* prog, const WalkShape& sh, size_t B, const u64* inputs, const u64* testvs, u64* wires_out, u64* gate_cts_out,
                  u64* out_cts, int on_device, Tables&& tables, Bootstrap&& bootstrap) {
    vpbs_ctx* ctx = sh.ctx;
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = sh.n_lwe + 1;
    const size_t n = (size_t)1 << sh.prm.log_N, kn = sh.prm.K * n, n_outs = prog->n_outs, rows_g = B * n_gates, rows_w = B * (n_in + n_outs);
    const bool multi = prog->multi;
    const std::vector<u32>& lf = prog->level_first;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            const WalkTables T = tables(mem, s);
            u64* d_wires = mem.words(rows_w * words);
            u64* d_cts = mem.words(rows_g * words);
            u64* d_out = out_cts || multi ? mem.words(rows_g * kn) : nullptr;   // multi: the wires are extracted from it
            u64* d_tv = mem.words(std::max<size_t>(1, std::min<size_t>(sh.max_batch, B * prog->widest)) * n);
            const u64 *d_testvs = testvs, *d_inputs = inputs;
            if (!on_device && n_gates) {
                u64* d = mem.words((size_t)prog->n_luts * n);
                VPBS_HIP(hipMemcpyAsync(d, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
                d_testvs = d;
            }
            if (n_in && !T.in_map) {   // the block of inputs as given
                VPBS_HIP(hipMemcpyAsync(d_wires, inputs, 8 * B * n_in * words, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
            } else if (n_in) {
                if (!on_device) {
                    u64* d = mem.words(B * n_in * words);
                    VPBS_HIP(hipMemcpyAsync(d, inputs, 8 * B * n_in * words, hipMemcpyHostToDevice, s));
                    d_inputs = d;
                }
                launch_gather(s, d_inputs, T.in_map, words, (unsigned)(B * n_in), d_wires);
                VPBS_HIP(hipGetLastError());
            }
            for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
                const size_t w = lf[lv + 1] - lf[lv], rows = B * w, base = B * lf[lv];
                for (size_t r0 = 0; r0 < rows; r0 += sh.max_batch) {
                    const unsigned c = (unsigned)std::min<size_t>(sh.max_batch, rows - r0);
                    u64* cts = d_cts + (base + r0) * words;
                    combine_enqueue(ctx, prog, prog->d_perm, d_wires, B, (unsigned)r0, lf[lv], (unsigned)w, c, words, sh.prm.log_N, cts);
                    launch_gather(s, d_testvs, T.lut + base + r0, n, c, d_tv);
                    VPBS_HIP(hipGetLastError());
                    if (!multi) {   // lwe_out: a contiguous piece of the level's block
                        bootstrap(cts, c, d_tv, base + r0, d_out ? d_out + (base + r0) * kn : nullptr, d_wires + (B * n_in + base + r0) * words);
                        continue;
                    }
                    // out_ct only; the chunk's output rows (a contiguous piece of the level's block of outputs) are extracted from it behind the launch
                    bootstrap(cts, c, d_tv, base + r0, d_out + (base + r0) * kn, nullptr);
                    const size_t o0 = prog->out_row(B, lv, r0), o1 = prog->out_row(B, lv, r0 + c);
                    vpbs::Timed t(ctx, "lwe_extract_at");
                    lwe_extract_at_enqueue(s, d_out, T.ext + o0, T.ext + B * n_outs + o0, sh.prm.log_N, sh.prm.K, sh.n_lwe, o1 - o0,
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
            deliver(wires_out, d_wires, T.wire_map, words, rows_w);
            deliver(gate_cts_out, d_cts, T.gate_map, words, rows_g);
            deliver(out_cts, out_cts ? d_out : nullptr, T.gate_map, kn, rows_g);
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

// vpbs_program_run; `b`'s runs are serialised by the caller
long program_run(vpbs_program* prog, vpbs_bootstrapper* b, const u64* inputs, const u64* testvs, u64* wires_out, u64* gate_cts_out, u64* out_cts,
                 int on_device) {
    if (!prog || !b || !prog->ctx) return VPBS_ERR_INVALID;
    BootstrapperShape sh{};
    bootstrapper_shape(b, &sh);
    vpbs_ctx* ctx = sh.ctx;
    if (ctx->device != prog->ctx->device) return ctx->err = "the program and the Bootstrapper are on different devices", VPBS_ERR_INVALID;
    if ((prog->n_inputs && !inputs) || (prog->n_gates && !testvs)) return ctx->err = "null inputs or testvs", VPBS_ERR_INVALID;
    {
        std::string msg;
        if (!slots_fit(prog, sh.prm.log_N, &msg)) return ctx->err = msg, VPBS_ERR_INVALID;
    }
    // one instance: the level-major table is the permuted wire table, and its index tables have been on the device since create
    return program_walk(
        prog, WalkShape{ctx, sh.prm, sh.n_lwe, sh.max_batch}, 1, inputs, testvs, wires_out, gate_cts_out, out_cts, on_device,
        [&](Scratch&, hipStream_t) { return WalkTables{prog->d_perm.lut, nullptr, prog->d_wire_pos, prog->d_gate_pos, prog->d_perm.ext}; },
        [&](const u64* d_cts, unsigned c, const u64* d_tv, size_t, u64* d_out_ct, u64* d_lwe_out) {
            bootstrapper_enqueue(b, d_cts, c, d_tv, 1, d_out_ct, d_lwe_out, nullptr);
        });
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
    const size_t n_outs = prog->n_outs, n_wires = (size_t)n_in + n_outs, B = instances;
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
    const size_t chunk_max = std::max<size_t>(1, std::min<size_t>(sh.max_batch, B * prog->widest)), rows_g = B * n_gates, rows_w = B * n_wires;
    const bool want_gates = gate_cts_out || out_cts;
    // identity [chunk_max] | key_of of every gate row | gate_lut of every gate row | input rows | caller's wire rows | caller's gate rows
    // multi: | extraction index of every output row | its gate row -- both in the order of the level-major block of outputs
    const size_t o_key = chunk_max, o_lut = o_key + rows_g, o_in = o_lut + rows_g, o_wire = o_in + B * n_in,
                 o_gate = o_wire + (wires_out ? rows_w : 0), o_ext = o_gate + (want_gates ? rows_g : 0), total = o_ext + (multi ? 2 * B * n_outs : 0);
    std::vector<u32> idx(total);   // lives until the wait
    if (multi)
        for (unsigned lv = 0; lv < prog->n_levels; ++lv) {
            const size_t w = lf[lv + 1] - lf[lv];
            for (size_t r = 0; r < B * w; ++r) {
                const size_t o = prog->out_row(B, lv, r), m = pof[lf[lv] + r % w + 1] - pof[lf[lv] + r % w];
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
                const size_t o = prog->out_row(B, lv, (size_t)pos_of[b] * (lf[lv + 1] - lf[lv]) + (gate_pos[g] - lf[lv]));
                for (u32 j = prog->out_first[g]; j < prog->out_first[g + 1]; ++j)
                    idx[o_wire + b * n_wires + n_in + j] = (u32)(B * n_in + o + (j - prog->out_first[g]));
            }
        }
        if (want_gates)
            for (unsigned g = 0; g < n_gates; ++g) idx[o_gate + b * n_gates + g] = (u32)gate_row(b, g);
    }
    const u32* d_idx = nullptr;
    return program_walk(
        prog, WalkShape{ctx, sh.prm, sh.n_lwe, sh.max_batch}, B, inputs, testvs, wires_out, gate_cts_out, out_cts, on_device,
        [&](Scratch& mem, hipStream_t s) {   // once, before the first launch
            u32* d = reinterpret_cast<u32*>(mem.words((total + 1) / 2));
            VPBS_HIP(hipMemcpyAsync(d, idx.data(), sizeof(u32) * total, hipMemcpyHostToDevice, s));
            d_idx = d;
            return WalkTables{d + o_lut, d + o_in, d + o_wire, d + o_gate, d + o_ext};
        },
        // the rows are in slot order already: the identity as `order`, the rows' own slots as `key_of`
        [&](const u64* d_cts, unsigned c, const u64* d_tv, size_t row, u64* d_out_ct, u64* d_lwe_out) {
            keyring_enqueue(ring, d_cts, c, d_tv, 1, d_idx, d_idx + o_key + row, d_out_ct, d_lwe_out, nullptr);
        });
}
// ---- the statement on the device: what every verifier recomputes before it looks at a proof ----
struct Statement {
    u64 *d_wires, *d_out, *d_cts, *d_testvs;   // the caller-order wire table, the claimed GLWEs [B n_gates][K N], the gate inputs, the test vectors
};
// The extraction of every output row b * n_outs + o of B instances of a multi-output program: index [B n_outs] | claimed GLWE [B n_outs].
// Empty for one instance (the program's resident table says the same) and for a program that is not multi.  A host array that
// statement_enqueue uploads: it lives until the caller's wait.
std::vector<u32> statement_ext(const vpbs_program* prog, size_t B) {
    std::vector<u32> ext;
    if (!prog->multi || B == 1) return ext;
    const size_t n_outs = prog->n_outs;
    ext.resize(2 * B * n_outs);
    for (size_t b = 0; b < B; ++b)
        for (size_t g = 0; g < prog->n_gates; ++g)
            for (u32 o = prog->out_first[g]; o < prog->out_first[g + 1]; ++o) {
                ext[b * n_outs + o] = o - prog->out_first[g];
                ext[B * n_outs + b * n_outs + o] = (u32)(b * prog->n_gates + g);
            }
    return ext;
}
// Queued on the context's stream, no wait: the upload of inputs [B][n_in], claimed outputs [B][n_gates] and test vectors [n_luts] (host
// arrays), ONE extraction launch over all claimed outputs, ONE combine launch over all rows (instance, gate) in the caller's order.  The
// shape has been checked (extraction_shape, slots_fit), B >= 1 and n_gates >= 1; the caller holds the device.  Throws DeviceError.
Statement statement_enqueue(const vpbs_program* prog, vpbs_ctx* ctx, Scratch& mem, unsigned log_n, unsigned K, unsigned n_lwe, const u64* inputs,
                            size_t B, const u64* out_cts, const u64* testvs, const std::vector<u32>& ext) {
    const unsigned n_in = prog->n_inputs, n_gates = prog->n_gates, words = n_lwe + 1;
    const size_t n = (size_t)1 << log_n, kn = K * n, n_outs = prog->n_outs, rows = B * n_gates;
    hipStream_t s = ctx->stream;
    Statement st{mem.words(B * (n_in + n_outs) * words), mem.words(rows * kn), mem.words(rows * words), mem.words((size_t)prog->n_luts * n)};
    if (n_in) VPBS_HIP(hipMemcpyAsync(st.d_wires, inputs, 8 * B * n_in * words, hipMemcpyHostToDevice, s));
    VPBS_HIP(hipMemcpyAsync(st.d_out, out_cts, 8 * rows * kn, hipMemcpyHostToDevice, s));
    VPBS_HIP(hipMemcpyAsync(st.d_testvs, testvs, 8 * (size_t)prog->n_luts * n, hipMemcpyHostToDevice, s));
    u64* d_extracted = st.d_wires + B * n_in * words;
    if (!prog->multi) {
        lwe_extract_enqueue(s, st.d_out, log_n, K, n_lwe, rows, d_extracted);
    } else {   // every (instance, gate, j) row in one launch
        const u32* d_ext = prog->d_given.ext;
        if (!ext.empty()) {
            u32* d = reinterpret_cast<u32*>(mem.words(ext.size() / 2));
            VPBS_HIP(hipMemcpyAsync(d, ext.data(), sizeof(u32) * ext.size(), hipMemcpyHostToDevice, s));
            d_ext = d;
        }
        lwe_extract_at_enqueue(s, st.d_out, d_ext, d_ext + B * n_outs, log_n, K, n_lwe, B * n_outs, d_extracted);
    }
    combine_enqueue(ctx, prog, prog->d_given, st.d_wires, B, 0, 0, n_gates, (unsigned)rows, words, log_n, st.d_cts);
    VPBS_HIP(hipGetLastError());
    return st;
}

// The proof check behind vpbs_program_verify (B = 1, key_of null: every row takes entry 0 of the key table) and vpbs_program_verify_batch,
// after their checks (offsets that do not decrease, rows >= 1): the statement, then the rows where they lie to the verifier's core in chunks
// of max_batch -- a chunk may straddle instances: every row brings its own indices -- with one wait per chunk for the result bytes.
// -> the number of accepted proofs, or the status of a refused chunk.  Throws DeviceError after the core has been told (pbs_verify_abandon).
long verify_rows(const vpbs_program* prog, PbsVerifyCore* core, const u64* d_key_table, vpbs_ctx* ctx, unsigned log_n, unsigned K, unsigned n_lwe,
                 size_t max_batch, const u64* inputs, size_t B, const u32* key_of, const u64* testvs, const u64* out_cts, const uint8_t* proofs,
                 const size_t* offsets, uint8_t* verdicts, uint8_t* reasons, uint8_t* proof_reasons) {
    const size_t n_gates = prog->n_gates, rows = B * n_gates, words = (size_t)n_lwe + 1, kn = (size_t)K << log_n;
    // key_of of every row | B > 1: testv_of = gate_lut tiled (one instance reads the program's resident gate_lut); uploaded once
    std::vector<u32> idx((B > 1 ? 2 : 1) * rows, 0);
    for (size_t r = 0; r < rows; ++r) {
        if (key_of) idx[r] = key_of[r / n_gates];
        if (B > 1) idx[rows + r] = prog->given.lut[r % n_gates];
    }
    const std::vector<u32> ext = statement_ext(prog, B);   // both live until the last wait
    long accepted = 0;
    VPBS_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch mem(ctx);
    try {
        const Statement st = statement_enqueue(prog, ctx, mem, log_n, K, n_lwe, inputs, B, out_cts, testvs, ext);
        u32* d_idx = reinterpret_cast<u32*>(mem.words((idx.size() + 1) / 2));
        VPBS_HIP(hipMemcpyAsync(d_idx, idx.data(), sizeof(u32) * idx.size(), hipMemcpyHostToDevice, s));
        const u32* d_testv_of = B > 1 ? d_idx + rows : prog->d_given.lut;
        for (size_t r0 = 0; r0 < rows; r0 += max_batch) {
            const size_t c = std::min(max_batch, rows - r0);
            const int rc = pbs_verify_enqueue(core, proofs, offsets + r0, c, st.d_cts + r0 * words, st.d_out + r0 * kn, st.d_testvs, d_testv_of + r0,
                                              d_key_table, d_idx + r0);
            if (rc) {
                (void)vpbs::stream_sync(s);
                return rc;
            }
            accepted += pbs_verify_collect(core, c, verdicts + r0, reasons ? reasons + r0 : nullptr, proof_reasons ? proof_reasons + r0 : nullptr);
        }
    } catch (const DeviceError& e) {
        pbs_verify_abandon(core, e);
        (void)vpbs::stream_sync(s);
        throw;
    }
    return accepted;
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
    G.slots.assign(n_gates, 0);
    if (described) std::copy(slots_in, slots_in + n_gates, G.slots.begin());
    // the caller's order reads a table with ALL outputs in one block behind the inputs
    for (size_t t = 0; t < T; ++t) {
        const u32 w = G.src[t];
        if (w < n_in) G.loc.insert(G.loc.end(), {0u, n_in, w});
        else G.loc.insert(G.loc.end(), {n_in, n_outs, w - n_in});
    }
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
    for (unsigned lv = 0; lv < p->n_levels; ++lv) p->widest = std::max(p->widest, p->level_first[lv + 1] - p->level_first[lv]);
    if (ctx) {
        Csr R;   // the permuted description: one block of outputs per level
        std::vector<u32> given_ext(2 * (size_t)n_outs), perm_ext(2 * (size_t)n_outs);   // multi: the extraction of every output row, both orders
        R.first.push_back(0);
        for (unsigned q = 0; q < n_gates; ++q) {
            const unsigned g = p->order[q];
            for (u64 t = G.first[g]; t < G.first[g + 1]; ++t) {
                const u32 row = wire_pos[G.src[t]];
                R.src.push_back(row);
                R.coef.push_back(G.coef[t]);
                if (row < n_in) {
                    R.loc.insert(R.loc.end(), {0u, n_in, row});
                } else {
                    const unsigned lv = p->level[gate_of[G.src[t] - n_in]] - 1;
                    const u32 o0 = pof[p->level_first[lv]], o1 = pof[p->level_first[lv + 1]];   // the level's block of outputs
                    R.loc.insert(R.loc.end(), {n_in + o0, o1 - o0, row - n_in - o0});
                }
            }
            R.first.push_back(R.coef.size());
            R.cst.push_back(G.cst[g]);
            R.lut.push_back(G.lut[g]);
            R.slots.push_back(G.slots[g]);
            for (u32 j = 0; j < out_first[g + 1] - out_first[g]; ++j) {
                given_ext[out_first[g] + j] = perm_ext[pof[q] + j] = j;
                given_ext[n_outs + out_first[g] + j] = g;
                perm_ext[n_outs + pof[q] + j] = q;
            }
        }
        p->ctx = ctx;
        try {
            VPBS_HIP(hipSetDevice(ctx->device));
            p->d_given = p->upload(G, given_ext, false);
            p->d_perm = p->upload(R, perm_ext, true);
            p->d_wire_pos = p->upload(wire_pos);
            p->d_gate_pos = p->upload(gate_pos);
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
    if (ctx->device != prog->ctx->device) return ctx->err = "the program and the verifier are on different devices", VPBS_ERR_INVALID;
    if (prog->n_gates == 0) return 0;
    if ((prog->n_inputs && !inputs) || !testvs || !out_cts || !proofs) return ctx->err = "null inputs, testvs, out_cts or proofs", VPBS_ERR_INVALID;
    unsigned log_n = 0;
    if (!extraction_shape(sh.N, sh.K, sh.n_lwe, &log_n))
        return ctx->err = "the verifier's shape has no sample extraction (N a power of two, 1 <= n_lwe <= (K - 1) N)", VPBS_ERR_INVALID;
    {
        std::string msg;
        if (!slots_fit(prog, log_n, &msg)) return ctx->err = msg, VPBS_ERR_INVALID;
    }
    for (unsigned g = 0; g < prog->n_gates; ++g)
        if (offsets[g + 1] < offsets[g]) return VPBS_ERR_INVALID;   // before anything is queued
    try {   // one instance on the verifier's own core and its key table of one entry
        return verify_rows(prog, pbs_verifier_core(pbs_verifier), pbs_verifier_key_table(pbs_verifier), ctx, log_n, sh.K, sh.n_lwe, sh.max_batch, inputs,
                           1, nullptr, testvs, out_cts, proofs, offsets, verdicts, reasons, proof_reasons);
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
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
    const unsigned n_in = prog->n_inputs;
    const size_t n_wires = (size_t)n_in + prog->n_outs, B = instances, rows = B * prog->n_gates;
    if (ctx->device != prog->ctx->device) return refuse(who + ": the program and the ring verifier are on different devices");
    if (n_wires && B > 0x7fffffffull / n_wires) return refuse(who + ": instances x wires exceeds 2^31 - 1 rows");
    if (B && !key_of) return refuse(who + ": null key_of");
    if (rows && ((n_in && !inputs) || !testvs || !out_cts || !proofs || !offsets || !verdicts))
        return refuse(who + ": null inputs, testvs, out_cts, proofs, offsets or verdicts");
    unsigned log_n = 0;
    if (!extraction_shape(sh.N, sh.K, sh.n_lwe, &log_n))
        return refuse(who + ": the verifier's shape has no sample extraction (N a power of two, 1 <= n_lwe <= (K - 1) N)");
    std::string msg;
    if (!slots_fit(prog, log_n, &msg)) return refuse(who + ": " + msg);
    if (!ring_verifier_check_slots(ring_verifier, key_of, B, who.c_str(), "instance", &msg)) return refuse(msg);
    for (size_t r = 0; r < rows; ++r)
        if (offsets[r + 1] < offsets[r]) return refuse(who + ": offsets decrease at row " + std::to_string(r));
    if (rows == 0) return 0;
    try {
        const long rc = verify_rows(prog, ring_verifier_core(ring_verifier), ring_verifier_key_table(ring_verifier), ctx, log_n, sh.K, sh.n_lwe,
                                    sh.max_batch, inputs, B, key_of, testvs, out_cts, proofs, offsets, verdicts, reasons, proof_reasons);
        if (rc < 0) report(err, err_len, who + ": malformed offsets");
        return rc;
    } catch (const DeviceError& e) {
        report(err, err_len, who + ": " + e.what);
        return e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
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
    const size_t kn = (size_t)sh.K * sh.N, n_wires = (size_t)n_in + prog->n_outs, B = instances, rows = B * n_gates;
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
    const std::vector<u32> ext = statement_ext(prog, B);   // lives until the last wait
    long accepted = 0;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch mem(ctx);
        try {
            const Statement st = statement_enqueue(prog, ctx, mem, log_n, sh.K, sh.n_lwe, inputs, B, out_cts, testvs, ext);
            u64* d_khs = mem.words(4 * n_keys);
            VPBS_HIP(hipMemcpyAsync(d_khs, key_hashes, 32 * n_keys, hipMemcpyHostToDevice, s));
            // the verifier's stages follow on the same stream: the tables stay where they are
            for (size_t b0 = 0; b0 < B; b0 += per) {
                const size_t c = std::min(per, B - b0), r0 = b0 * n_gates;
                const long rc = vpbs_aggregate_verifier_run_many(agg_verifier, bytes, offsets + b0, c, leaf_first.data(), st.d_testvs, prog->n_luts,
                                                                 lut_of.data(), st.d_cts + r0 * words, st.d_out + r0 * kn, d_khs, n_keys, key_row.data() + r0, 1,
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

// Prover context: one device, one HIP stream, a size-keyed device-memory pool (steady-state step proofs allocate
// nothing), cached twiddle / coset-power tables, and optional per-kernel HIP-event timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/vpbs_prover.h"
#include "kernels.h"

namespace vpbs {
struct DeviceError {
    int status;
    std::string what;
};

// The call that REPORTS a failure clears it: the waits only peek at the thread's pending error (vpbs::stream_sync), so that the
// stage-end checks still see a failed launch -- but once it has been turned into a DeviceError, and from there into the status and
// vpbs_last_error() of the entry point, it is consumed here.  A non-sticky failure (bad configuration, out of resources; this library's or
// another one's on the same thread) is thus reported by exactly one call; a C++ or Rust host needs no hipGetLastError of its own to go on.
#define VPBS_HIP(expr)                                                                                         \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            (void)hipGetLastError();                                                                           \
            throw ::vpbs::DeviceError{e_ == hipErrorOutOfMemory ? VPBS_ERR_OOM : VPBS_ERR_DEVICE,              \
                                      std::string(#expr) + ": " + hipGetErrorString(e_)};                      \
        }                                                                                                      \
    } while (0)
#define VPBS_REQUIRE(cond, msg)                                         \
    do {                                                                \
        if (!(cond)) throw ::vpbs::DeviceError{VPBS_ERR_INVALID, msg};  \
    } while (0)

// a message into the caller's buffer of an entry point that takes (err, err_len): truncated, always terminated; a null buffer takes nothing
inline void report(char* err, size_t err_len, const std::string& m) {
    if (err && err_len) {
        std::strncpy(err, m.c_str(), err_len - 1);
        err[err_len - 1] = 0;
    }
}
}  // namespace vpbs

namespace vpbs {
// How a host thread waits for its stream.  hipStreamSynchronize spins: the thread that proves a chain burns a whole CPU while the device
// works (measured, VPBS_TRACE_IVC: with four chains on TWO CPUs a proving thread used 16 ms of CPU per proof inside vpbs_prove_step, of which
// about one is work).  In blocking mode the wait polls hipStreamQuery and sleeps in between.  Process-wide (it is about the CPUs the process
// has): vpbs_host_set_blocking_sync, default from VPBS_BLOCKING_SYNC, else AUTO -- block when the process may use fewer than 8 CPUs.
int blocking_sync_mode();                 // 0 spin, 1 block
hipError_t stream_sync(hipStream_t s);    // drop-in for hipStreamSynchronize
void stream_sync_forget(hipStream_t s);   // before hipStreamDestroy: the stream's completion word (api.hip) is freed
int sync_word_mode();                     // 1: waits read a word the device writes (default); 0: they go through the runtime
// host->device copy on `s` and the wait for it; copy and marker are queued as one step, so a caller on a stream that several threads share
// waits for its own copy and for what was queued before it, never for a copy another thread queued behind it
hipError_t stream_upload_sync(hipStream_t s, void* d_dst, const void* host_src, size_t bytes);
// The streams the library holds per device (api.hip): a context's prover stream is counted from vpbs_ctx_create to vpbs_ctx_destroy, its
// gate-lane streams as they come and go; the last context to close takes the device's upload stream with it (the caller has selected the device).
void device_streams_note(int device, int contexts, int gate_lanes);
void device_stream_counts(int device, unsigned out[2]);   // {prover streams, auxiliary streams: upload stream + gate lanes}
// out[k] = hash_no_pad(h_{k-1} || items[k]), h_{-1} = prefix; concurrent callers with long items share the lanes of the eight-lane host Poseidon
void hash_links_shared(const u64 prefix[4], const u64* const* items, size_t n_links, size_t item_len, u64* out);
// The key hash chain of ONE key set, every link kept: links [n_lwe + 2][4] over the items [0^ggsw_len, bsk_0 .. bsk_{n-1}, ksk] from a zero
// prefix, as vpbs_verify_pbs hashes them, without materialising the items (bsk [n_lwe][ggsw_len] may be null for n_lwe = 0).  The last link
// is the key hash.  keys_on_device: bsk and ksk are device pointers and are downloaded once for this, with blocking copies on no stream of
// the library's (the caller holds the device); throws DeviceError for a failed copy.  Walked through hash_links_shared.
void key_hash_links(const u64* bsk, const u64* ksk, int keys_on_device, unsigned n_lwe, size_t ggsw_len, u64* links);
void blocking_sync_budget_changed();      // the process's CPU budget was set: AUTO decides again
}  // namespace vpbs

struct vpbs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;   // the one stream a context creates; vpbs_device_upload_bg goes through the device's shared upload stream (api.hip)
    unsigned log_n_max = 0, rate_bits = 3, cap_height = 4;
    vpbs::Tuning tune = vpbs::Tuning::from_env();   // vpbs_ctx_set_option
    vpbs_compat compat{0, 1, 1, 1};   // vpbs_compat_default: plonky2 0.2.0 as restated (include/vpbs_prover.h, the switch table)
    std::string err;

    // ---- device memory pool ----
    std::multimap<size_t, void*> free_blocks;
    std::unordered_map<void*, size_t> block_size;
    size_t pool_bytes = 0;
    void* alloc_bytes(size_t bytes);
    vpbs::u64* alloc_words(size_t words) { return static_cast<vpbs::u64*>(alloc_bytes(words * sizeof(vpbs::u64))); }
    void release(void* p);
    void trim();

    // ---- pinned staging for the small device->host results of the transcript (caps, openings, query records) ----
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // copy + stream synchronise; dst is ordinary (pageable) caller memory
    void d2h_sync(void* dst, const void* d_src, size_t bytes);
    void ensure_pinned();
    // a 4-byte device flag copied to pinned memory WITHOUT a synchronisation of its own: the value is there after the next d2h_sync (or
    // any synchronisation of the stream).  One flag in flight per context.  nullptr when no pinned memory could be had (the caller syncs).
    volatile unsigned* d2h_deferred_flag(const void* d_src);

    // ---- tables ----
    std::map<std::pair<unsigned, bool>, vpbs::u64*> root_tables;                 // (log_n, inverse)
    std::map<std::tuple<unsigned, unsigned, vpbs::u64>, vpbs::u64*> prescale_tables;  // (log_n, rate_bits, shift)
    std::map<std::tuple<unsigned, unsigned, vpbs::u64>, vpbs::u64*> lde_tables;       // (log_n, rate_bits, shift)
    std::map<unsigned, vpbs::u64*> ring_tables;  // log_N -> [ROOTS | INVROOTS] of the negacyclic NTT (params_{N}.rs), 2N words
    const vpbs::u64* ring_table(unsigned log_n_ring);
    std::map<unsigned, vpbs::u64*> l0_tables;  // log_n -> L_0 on the coset, leaf order
    const vpbs::u64* l0_table(unsigned log_n);
    const vpbs::u64* roots(unsigned log_n, bool inverse);
    const vpbs::u64* prescale(unsigned log_n, unsigned rate_bits, vpbs::u64 shift);    // plain powers (shift w_big^r)^i
    const vpbs::u64* lde_table(unsigned log_n, unsigned rate_bits, vpbs::u64 shift);   // what launch_coset_lde reads (kernels.h)

    // ---- helper streams for the gate-constraint kernels (created on first use) ----
    hipStream_t gate_streams[2] = {nullptr, nullptr};
    hipEvent_t gate_fork = nullptr, gate_join[2] = {nullptr, nullptr};
    void ensure_gate_lanes();
    // 1 (one stream): the default since the gate constraints run in the LDS-tile kernel -- its workgroups fill a CU's LDS and registers, so
    // the permutation part gains nothing beside it (9.67 vs 9.93 ms per step proof); 3: the helper streams of rounds 1-2, still the better
    // arrangement for the per-gate launches.  VPBS_GATE_LANES=3 in the environment makes that the default; vpbs_ctx_set_gate_lanes.
    unsigned gate_lanes = default_gate_lanes();
    static unsigned default_gate_lanes() {
        const char* e = getenv("VPBS_GATE_LANES");
        return e && atoi(e) == 3 ? 3u : 1u;
    }

    // ---- timing ----
    vpbs::u64* d_clock_samples = nullptr;   // [CLOCK_SAMPLES][2], one pair per leaf-hash launch while timing is on (ring)
    static constexpr unsigned CLOCK_SAMPLES = 1024;
    unsigned clock_samples = 0;
    vpbs::u64* next_clock_sample();         // nullptr unless timing is on
    bool timing = false;
    std::string timing_only;  // when non-empty, only this timer is recorded
    struct Pending {
        int name_id;
        hipEvent_t start, stop;
    };
    std::vector<std::string> timer_names;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<double, long>> totals;
    int timer_id(const char* name);
    hipEvent_t get_event();
    void resolve_timing();
};

namespace vpbs {
// RAII: HIP events around a group of launches on the ctx stream (no-op unless timing is enabled)
struct Timed {
    vpbs_ctx* c;
    int id = -1;
    hipEvent_t start = nullptr;
    Timed(vpbs_ctx* ctx, const char* name) : c(ctx) {
        if (!c->timing) return;
        if (!c->timing_only.empty() && c->timing_only != name) return;
        id = c->timer_id(name);
        start = c->get_event();
        (void)hipEventRecord(start, c->stream);
    }
    ~Timed() {
        if (id < 0) return;
        hipEvent_t stop = c->get_event();
        (void)hipEventRecord(stop, c->stream);
        c->pending.push_back({id, start, stop});
    }
};
}  // namespace vpbs

struct vpbs_batch {
    vpbs_ctx* ctx = nullptr;
    unsigned ncols = 0, log_n = 0;
    vpbs::u64* d_coeffs = nullptr;   // [ncols][n]
    vpbs::u64* d_lde = nullptr;      // [ncols][n << rate_bits], leaf order
    vpbs::u64* d_digests = nullptr;  // Merkle levels back to back
    std::vector<size_t> level_off;   // word offset of each level; last level = cap
    // coset sharding: this batch holds leaf blocks [shard * per, (shard + 1) * per) of the 2^rate_bits
    // blocks, per = 2^rate_bits / n_shards, i.e. the leaves [leaf_offset(), leaf_offset() + lde_len()) and the
    // cap entries [shard * cap_len(), (shard + 1) * cap_len()).  n_shards == 1: the whole commitment.
    unsigned shard = 0, n_shards = 1;
    size_t n() const { return (size_t)1 << log_n; }
    unsigned blocks() const { return (1u << ctx->rate_bits) / n_shards; }
    size_t lde_len() const { return n() * blocks(); }
    size_t leaf_offset() const { return (size_t)shard * lde_len(); }
    size_t cap_len() const { return ((size_t)1 << ctx->cap_height) / n_shards; }
    unsigned n_levels() const { return (unsigned)level_off.size(); }
};

namespace vpbs {
// The largest LDE any entry point takes is 2^MAX_LDE_BITS leaves (vpbs_ctx_create: log_n_max + rate_bits <= MAX_LDE_BITS).  A tree has
// log_leaves - cap_height + 1 levels, the leaves' digests and the cap included, and OpenTree::level_off (kernels.h) holds MAX_TREE_LEVELS of
// them: every tree of a context with cap_height >= 1, and with cap_height = 0 every tree but the one over the full 2^MAX_LDE_BITS leaves,
// which has one level more.  That tree can be committed, and its cap read; the calls that open it refuse it (set_tree_levels).
constexpr unsigned MAX_LDE_BITS = 24;
constexpr unsigned MAX_TREE_LEVELS = sizeof(OpenTree::level_off) / sizeof(size_t);
static_assert(MAX_TREE_LEVELS == MAX_LDE_BITS, "OpenTree::level_off is sized by the log_n_max + rate_bits limit of vpbs_ctx_create");
constexpr const char* TOO_MANY_TREE_LEVELS = "a Merkle tree of more than 24 levels cannot be opened (2^24 leaves under cap_height 0)";
static_assert(MAX_TREE_LEVELS == 24, "TOO_MANY_TREE_LEVELS names the limit");
// the one place that fills OpenTree::level_off and n_siblings; false, and nothing written, for a tree the array cannot hold
template <class Offsets> inline bool set_tree_levels(OpenTree& t, const Offsets& level_off) {
    if (level_off.empty() || level_off.size() > MAX_TREE_LEVELS) return false;
    for (size_t k = 0; k < level_off.size(); ++k) t.level_off[k] = level_off[k];
    t.n_siblings = (u32)level_off.size() - 1;
    return true;
}
// Merkle level layout for a tree with n_leaves leaves and cap height h: returns total words
size_t merkle_layout(size_t n_leaves, unsigned cap_height, std::vector<size_t>& level_off);
// commit a device-resident matrix (values or coefficients); returns a new batch
vpbs_batch* commit_device(vpbs_ctx* ctx, const u64* d_in, unsigned ncols, unsigned log_n, bool is_values, unsigned shard = 0,
                          unsigned n_shards = 1);
void batch_cap_to_host(vpbs_batch* b, u64* cap_out);
// vpbs_device_scatter's copy + kernel on the context's stream; wait = false: queued only (api.hip)
int device_scatter(vpbs_ctx* c, uint64_t* d_dst, const uint64_t* d_positions, const uint64_t* host_values, size_t count, uint64_t* d_stage, bool wait);
}  // namespace vpbs

// The worker pool of the batch provers: C chains of the device-witness pipeline (vpbs_ivc, csrc/ivc.hip) that take ciphertext indices from a
// queue.  Per ciphertext a worker thread lets its KEY SOURCE leave every intermediate accumulator of the chain on the device (they ARE the
// `current accumulator` public inputs of the n + 2 step proofs), walks the LWE hash chain on the host (one permutation per link) and proves
// the chain through vpbs::ivc_prove_pbs_resident: the early-phase preset matrix of every batch of steps is assembled on the device by the
// kernels of pbs_prove_pool.hip, straight from the resident sources --
//
//   preset rows of step s                     source
//   previous proof's words                    zeros (late presets: the early phase ignores them)
//   acc_init | counter                        (0, .., 0, testv) | s
//   accumulator                               the key source's accs[s - 1]             (zeros for s = 0)     TRANSPOSED [cnt][K N] -> [K N][cnt]
//   key hash | LWE hash                       resident key link s - 1 | the chain's LWE link s - 1  (zeros for s = 0)
//   verifier data, condition                  constant | s != 0
//   GGSW                                      zeros, resident bsk[s - 1], resident ksk                      TRANSPOSED [cnt][ggsw] -> [ggsw][cnt]
//   mask                                      ct[n], ct[s - 1], 0
//   own / dummy verifier data, dummy proof    constants of the object
//   the dummy proof's public inputs           zeros
//
// -- so neither the 16 384 words of bsk[s] per step nor anything else of the matrix is stored by a host thread or crosses PCIe.
//
// A RESUMED chain (vpbs_pbs_prover_resume, vpbs_ring_prover_resume) enters this at step k of its checkpoint: open_checkpoints validates every
// checkpoint on the host before anything is queued (the key hash against the resident link k - 1: the pool holds every link, so no key
// chain is walked), the key source leaves accumulators k - 1 .. n + 1 through the kernels' start mode, and ivc_prove_pbs_resident goes on
// at step k with the checkpoint's proof words and public inputs; the table above is read at rows s >= k only.
//
// The pool is parameterised by its key source: which resident key set (device bsk and ksk, the key hash chain on the host and on the
// device) the chain of ciphertext i is proven under, a function that leaves that ciphertext's accumulators on the device, and one that makes
// a block of a run's outputs.  One key set and a Bootstrapper: vpbs_pbs_prover (pbs_prove_batch.hip).  The slot key_of[i] of a key ring:
// vpbs_ring_prover (pbs_prove_ring.hip).  What the two owners do alike is stated here once and defined in pbs_prove_pool.hip, the one file
// that compiles the two kernels: creation, the run behind run and resume of both, and the entry points that only pass through.
// Library-internal.
#pragma once
#include <algorithm>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "context.h"
#include "ivc_resident.h"

namespace vpbs {
struct PresetArgs {
    u64* m;                 // [n_preset][cnt], instances innermost
    const u64* testv;       // [N]
    const u64* accs;        // [n_lwe + 2][K N]
    const u64* key_links;   // [n_lwe + 2][4]
    const u64* lwe_links;   // [n_lwe + 2][4]
    const u64* ct;          // [n_lwe + 1]
    const u64* bsk;         // [n_lwe][ggsw_len]
    const u64* ksk;         // [ggsw_len]
    const u64* consts;      // own verifier data [vk] | dummy verifier data [vk] | dummy proof [proof_words]
    unsigned first, cnt, n_lwe, N;
    size_t kn, proof_words, n_pi, ggsw_len, vk_words;
    // first rows of the sections (the PartialWitness order of vpbs_ivc_create)
    __host__ __device__ size_t r_acc_init() const { return proof_words; }
    __host__ __device__ size_t r_counter() const { return proof_words + kn; }
    __host__ __device__ size_t r_acc() const { return proof_words + kn + 1; }
    __host__ __device__ size_t r_hashes() const { return proof_words + 2 * kn + 1; }
    __host__ __device__ size_t r_own_vk() const { return proof_words + 2 * kn + 9; }
    __host__ __device__ size_t r_cond() const { return proof_words + n_pi; }
    __host__ __device__ size_t r_ggsw() const { return proof_words + n_pi + 1; }
    __host__ __device__ size_t r_mask() const { return r_ggsw() + ggsw_len; }
    __host__ __device__ size_t r_consts() const { return r_mask() + 1; }
    __host__ __device__ size_t r_dummy_pis() const { return r_consts() + 2 * vk_words + proof_words; }
    __host__ __device__ size_t n_preset() const { return r_dummy_pis() + n_pi; }
    __host__ __device__ size_t plain_rows() const { return n_preset() - kn - ggsw_len; }   // all but the accumulator and the GGSW
};

// preset_rows_kernel and preset_transpose_kernel queued on s; the caller orders and waits
void launch_preset(hipStream_t s, const PresetArgs& a);

// the resident key set a chain is proven under
struct KeySource {
    const u64 *d_bsk = nullptr, *d_ksk = nullptr;   // device: [n_lwe][ggsw_len], [ggsw_len]
    const u64* d_key_links = nullptr;               // device [n_lwe + 2][4]
    const u64* key_links = nullptr;                 // host   [n_lwe + 2][4]
};

struct ProvePool;
// An owner as its entry points hand it on: the pool and the mutex of its runs, both null for a null object.  Either owner names its two
// members `pool` and `run_mu`.
struct PoolRef {
    ProvePool* pool = nullptr;
    std::mutex* run_mu = nullptr;
};
template <class Owner>
PoolRef pool_ref(const Owner* p) {
    return p ? PoolRef{const_cast<ProvePool*>(&p->pool), const_cast<std::mutex*>(&p->run_mu)} : PoolRef{};
}

struct ProvePool {
    struct Worker {   // one chain in flight: a context, a vpbs_ivc in the device-witness pipeline, the chain's public inputs
        ProvePool* pool = nullptr;
        vpbs_ctx* ctx = nullptr;
        vpbs_ivc* ivc = nullptr;
        u64 *d_accs = nullptr, *d_lwe_links = nullptr, *d_ct = nullptr, *d_testv = nullptr;   // device (the bootstrap context's pool)
        u64* d_acc_in = nullptr;   // device [K N]: a resumed chain's accumulator after step k - 1, from its checkpoint
        u64* accs = nullptr;   // pinned host [n_lwe + 2][K N]
        std::vector<u64> lwe_links;
        std::vector<uint8_t> proof;
        size_t index = 0;   // the ciphertext being proven
        KeySource keys;     // of that ciphertext
    };
    static constexpr size_t OUT_BATCH = 256;   // rows per launch of a run's outputs: the max_batch of the owner's Bootstrapper or key ring
    int device = 0;
    unsigned n_lwe = 0, total = 0;
    IvcShape shape{};
    vpbs_ctx* boot_ctx = nullptr;   // made by create: the key source computes on its stream, the workers' device buffers are from its pool
    std::mutex boot_mu;             // one chain at a time takes its public inputs from the key source
    u64* d_consts = nullptr;
    std::vector<u64*> owned;        // device memory of the bootstrap context's pool
    std::vector<Worker> workers;
    size_t max_bytes = 0;
    // ---- the key source (set by the owner before the first chain) ----
    std::function<KeySource(size_t index)> keys_of;   // the key set of ciphertext `index` of the run
    // w.d_ct and w.d_testv are queued on boot_ctx's stream: leave the n + 2 accumulators of that ciphertext in w.d_accs, complete or queued on
    // the same stream; false with a message otherwise.  from > 0 (a resumed chain): w.d_acc_in is queued too and holds the accumulator after
    // step from - 1; a count-1 run_from leaves slots from - 1 .. n + 1, the slots below keep the worker's previous chain and are read by
    // nobody (preset_*_kernel for step s >= from reads entry s - 1 >= from - 1 only).  Called under boot_mu.
    std::function<bool(Worker& w, unsigned from, std::string& why)> accumulators;
    // The outputs of rows i0 .. i0 + c of a run (c <= OUT_BATCH), every pointer already at row i0: one run_from launch of the owner's
    // Bootstrapper or ring, start and acc_in null when no row of the block is resumed -> the launch's status (c when all is well).  A
    // failure is reported as "<outputs_name>[_from]: <the bootstrap context's last error>".  Called under boot_mu.
    std::function<long(size_t i0, size_t c, const u64* cts, const uint32_t* start, const u64* acc_in, const u64* testv, int testv_per_ct,
                       u64* out_ct, u64* lwe_out)> outputs;
    const char* outputs_name = "";   // "vpbs_bootstrapper_run", "vpbs_keyring_run"
    // ---- a run ----
    std::mutex cb_mu;                // callbacks never two at once
    vpbs_pbs_run_stats stats{};      // of the last run
    vpbs_pbs_checkpoint_fn ckpt_fn = nullptr;
    void* ckpt_user = nullptr;
    // the checkpoints of a resume, row by row: opened[i].k = 0 for a row that starts at step 0 (none given, or refused); refused[i] is the
    // message of a refused one ("checkpoint: <why>"), empty otherwise
    struct Resume {
        const uint8_t* const* bytes = nullptr;
        const size_t* lens = nullptr;
        std::vector<IvcCheckpoint> opened;
        std::vector<std::string> refused;
        size_t resumed = 0;   // rows accepted
        const u64* acc_of(size_t i, size_t kn) const { return opened[i].pis.data() + kn + 1; }
    };

    ~ProvePool();
    // What both *_create entry points begin with: their refusals (the owner has checked its own pointers), the bootstrap context, then
    // `before_chains` if given (the ring prover makes its ring there: its refusals cost nothing, the chains are the large allocations) and
    // the chains, which are what tools/prove_ivc.py builds per chain.  VPBS_OK, or a status with a message; the pool frees what it made.
    int create(int device_ordinal, const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, const vpbs_tfhe_params* prm, unsigned n_lwe,
               unsigned chains, unsigned witness_batch, char* err, size_t err_len, const std::function<int()>& before_chains = nullptr);
    u64* alloc(size_t words) {
        u64* d = boot_ctx->alloc_words(std::max<size_t>(1, words));
        owned.push_back(d);
        return d;
    }
    // the constants of every step and the workers' buffers, queued on boot_ctx's stream, and the wait for that stream (so what the owner
    // queued there before is complete too); VPBS_OK, or a status with a message
    int alloc_buffers(char* err, size_t err_len);
    // the chains and the device memory, before the owner frees what else lives in boot_ctx; the destructor then frees boot_ctx
    void destroy();
    PresetArgs preset_args(const Worker& w, unsigned first, unsigned cnt, u64* d_matrix) const;
    // the chain's public inputs where ivc_prove_pbs_resident wants them: accumulators on the device (the key source, this worker's buffer) and
    // on the host (one copy of (n + 2) K N words), the LWE hash chain on both.  Under boot_mu, on the bootstrap context's stream.
    // from > 0: a resumed chain; acc_from [K N] (host) is the accumulator after step from - 1, and only entries from - 1 .. n + 1 of the
    // accumulators are made and copied.  The LWE links are walked from 0 all the same (730 permutations).
    int prepare_chain(Worker& w, const u64* ct, const u64* testv, std::string& why, unsigned from = 0, const u64* acc_from = nullptr);
    // The checkpoints of a resume, validated on the host before anything is queued, the rows spread over the worker threads (each uses its
    // own chain's vpbs_ivc, read-only): ivc_open_checkpoint (the prefix form of verify_pbs against the object's own verifier data, LWE hash
    // chain included), the counter against `steps`, then the key hash against link k - 1 of the row's resident key set -- one 32-byte
    // compare; no key chain is walked.  keys_of must answer for the run already.
    void open_checkpoints(const u64* cts, size_t count, const u64* testv, int testv_per_ct, const uint8_t* const* checkpoints, const size_t* lens,
                          unsigned steps, Resume& rs);
    // start [c] and acc_in [c][K N] of the rows i0 .. i0 + c of a resume for a run_from launch; false when none of them is resumed
    bool start_rows(const Resume& rs, size_t i0, size_t c, std::vector<uint32_t>& start, std::vector<u64>& acc_in) const;
    // the proofs of a run whose outputs are complete (stats.outputs_seconds is set; t_call: when the owner's run began): workers take
    // ciphertext indices from a queue; one that fails reports and takes the next, nobody waits for anybody.  Returns the proofs delivered.
    // rs (a resume): a refused row reports its message and is not proven; an accepted one goes on at its checkpoint's step.
    long prove(const u64* cts, size_t count, const u64* testv, int testv_per_ct, unsigned steps, double t_call, vpbs_pbs_proof_fn proof_fn,
               void* user, const Resume* rs = nullptr);

    // ---- the entry points of both owners ----
    // What every run and resume entry refuses before it takes a lock, in the order it always did: 1 when the run may start, 0 for an empty
    // batch, VPBS_ERR_INVALID with a message otherwise.  key_of: null for the owner that has none, else the address of the caller's.
    static long check_run(PoolRef r, const u64* cts, size_t count, const u64* testv, const uint32_t* const* key_of,
                          const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, vpbs_pbs_proof_fn proof_fn, char* err, size_t err_len);
    // A run (checkpoints = null) or a resume that check_run let pass, under the owner's run mutex, the key source answering for these rows:
    // the checkpoints opened, every output (one `outputs` block per OUT_BATCH rows), then the proofs.  Returns the proofs delivered.
    long run(const u64* cts, size_t count, const u64* testv, int testv_per_ct, const uint8_t* const* checkpoints, const size_t* lens, unsigned steps,
             u64* out_ct, u64* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len);
    // vpbs_*_prover_verifier_data, _set_check_witness, _witness_checks, _set_checkpoint and _last_run: VPBS_ERR_INVALID for a null object or
    // output, the run mutex where they change something
    static int verifier_data(PoolRef r, uint64_t* cyclic_vk, uint64_t* dummy_vk);
    static int set_check_witness(PoolRef r, int on);
    static int witness_checks(PoolRef r, uint64_t out[2]);
    static int set_checkpoint(PoolRef r, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user);
    static int last_run(PoolRef r, vpbs_pbs_run_stats* out);
};
}  // namespace vpbs

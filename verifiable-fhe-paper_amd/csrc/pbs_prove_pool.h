// The worker pool of the batch provers: C chains of the device-witness pipeline (vpbs_ivc, csrc/ivc.hip) that take ciphertext indices from a
// queue.  Per ciphertext a worker thread lets its KEY SOURCE leave every intermediate accumulator of the chain on the device (they ARE the
// `current accumulator` public inputs of the n + 2 step proofs), walks the LWE hash chain on the host (one permutation per link) and proves
// the chain through vpbs::ivc_prove_pbs_resident: the early-phase preset matrix of every batch of steps is assembled on the device by the
// kernels below, straight from the resident sources --
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
// device) the chain of ciphertext i is proven under, and a function that leaves that ciphertext's accumulators on the device.  One key set
// and a Bootstrapper: vpbs_pbs_prover (pbs_prove_batch.hip).  The slot key_of[i] of a key ring: vpbs_ring_prover (pbs_prove_ring.hip).
// Everything here is in an unnamed namespace: the library is built without relocatable device code, so each of the two files that include
// this header gets the two kernels, and the pool that launches them, for itself.  Library-internal.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <mutex>
#include <pthread.h>
#include <string>
#include <thread>
#include <vector>

#include "context.h"
#include "ivc_resident.h"

namespace vpbs {
namespace {
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

// every row that is a broadcast or a short gather: one thread per word of those rows (the grid skips the two transposed blocks, which
// belong to preset_transpose_kernel and are most of the matrix), consecutive threads on consecutive instances of a row
__global__ void __launch_bounds__(256) preset_rows_kernel(PresetArgs a) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.plain_rows() * a.cnt) return;
    size_t r = q / a.cnt;   // among the plain rows; below: in the matrix
    if (r >= a.r_acc()) r += a.kn;
    if (r >= a.r_ggsw()) r += a.ggsw_len;
    const unsigned s = a.first + (unsigned)(q % a.cnt);
    u64 v = 0;
    if (r < a.r_acc_init()) {
        v = 0;
    } else if (r < a.r_counter()) {
        const size_t k = r - a.r_acc_init();
        v = k >= a.kn - a.N ? a.testv[k - (a.kn - a.N)] : 0;
    } else if (r == a.r_counter()) {
        v = s;
    } else if (r < a.r_own_vk()) {
        const size_t h = r - a.r_hashes();
        v = s == 0 ? 0 : (h < 4 ? a.key_links[(size_t)(s - 1) * 4 + h] : a.lwe_links[(size_t)(s - 1) * 4 + h - 4]);
    } else if (r < a.r_cond()) {
        v = a.consts[r - a.r_own_vk()];
    } else if (r == a.r_cond()) {
        v = s != 0;
    } else if (r == a.r_mask()) {
        v = s == 0 ? a.ct[a.n_lwe] : (s <= a.n_lwe ? a.ct[s - 1] : 0);
    } else if (r < a.r_dummy_pis()) {
        v = a.consts[r - a.r_consts()];
    }
    a.m[r * a.cnt + (q % a.cnt)] = v;
}

// The accumulator (blockIdx.z = 0) and the GGSW (1) of cnt consecutive steps: per step a contiguous source row, in the matrix one column.
// A workgroup turns a tile of 32 steps x 64 words in LDS: rows are read coalesced (64 lanes on 512 contiguous bytes), columns written
// coalesced (32 lanes on the 32 instances of a matrix row).  A tile row is padded by one word: the 32 lanes of a half-wave then read
// words 65 apart, i.e. banks 2 (i + k) and 2 (i + k) + 1 mod 64 -- all 64 banks, no conflict.
constexpr unsigned TILE_I = 32, TILE_K = 64;
__global__ void __launch_bounds__(256) preset_transpose_kernel(PresetArgs a) {
    __shared__ u64 tile[TILE_I][TILE_K + 1];
    const bool ggsw = blockIdx.z == 1;
    const size_t len = ggsw ? a.ggsw_len : a.kn, r0 = ggsw ? a.r_ggsw() : a.r_acc();
    const size_t k0 = (size_t)blockIdx.x * TILE_K;
    const unsigned i0 = blockIdx.y * TILE_I;
    if (k0 >= len) return;   // the grid is sized for the longer block (uniform per workgroup: before any barrier)
    for (unsigned ii = threadIdx.x / TILE_K; ii < TILE_I; ii += 256 / TILE_K) {
        const unsigned k = threadIdx.x % TILE_K, i = i0 + ii;
        u64 v = 0;
        if (i < a.cnt && k0 + k < len) {
            const unsigned s = a.first + i;
            const u64* src = s == 0 ? nullptr
                             : ggsw ? (s <= a.n_lwe ? a.bsk + (size_t)(s - 1) * a.ggsw_len : a.ksk)
                                    : a.accs + (size_t)(s - 1) * a.kn;
            if (src) v = src[k0 + k];
        }
        tile[ii][k] = v;
    }
    __syncthreads();
    for (unsigned k = threadIdx.x / TILE_I; k < TILE_K; k += 256 / TILE_I) {
        const unsigned ii = threadIdx.x % TILE_I;
        if (k0 + k < len && i0 + ii < a.cnt) a.m[(r0 + k0 + k) * a.cnt + i0 + ii] = tile[ii][k];
    }
}

// both kernels queued on s; the caller orders and waits
void launch_preset(hipStream_t s, const PresetArgs& a) {
    const size_t words = a.plain_rows() * a.cnt;
    hipLaunchKernelGGL(preset_rows_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a);
    const size_t longer = std::max(a.ggsw_len, a.kn);
    hipLaunchKernelGGL(preset_transpose_kernel, dim3((unsigned)((longer + TILE_K - 1) / TILE_K), (a.cnt + TILE_I - 1) / TILE_I, 2), dim3(256), 0, s, a);
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the resident key set a chain is proven under
struct KeySource {
    const u64 *d_bsk = nullptr, *d_ksk = nullptr;   // device: [n_lwe][ggsw_len], [ggsw_len]
    const u64* d_key_links = nullptr;               // device [n_lwe + 2][4]
    const u64* key_links = nullptr;                 // host   [n_lwe + 2][4]
};

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
    int device = 0;
    unsigned n_lwe = 0, total = 0;
    IvcShape shape{};
    vpbs_ctx* boot_ctx = nullptr;   // the owner's: the key source computes on its stream, the workers' device buffers are from its pool
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

    // the chains: what tools/prove_ivc.py builds per chain.  boot_ctx is set; VPBS_OK, or a status with a message
    int create_chains(const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, const vpbs_tfhe_params* prm, unsigned chains,
                      unsigned witness_batch, unsigned log_n_max, char* err, size_t err_len) {
        const unsigned N = 1u << prm->log_N, K = prm->K;
        const size_t ggsw_len = (size_t)K * prm->ELL * K * N;
        char e[512] = {0};
        workers.resize(chains);
        for (auto& w : workers) {
            w.pool = this;
            int rc = vpbs_ctx_create(device, log_n_max, 3, 4, &w.ctx);
            if (rc != VPBS_OK) return report(err, err_len, "a chain's context could not be made"), rc;
            // chains side by side hide latency: the one-lane Poseidon form down to 2048 nodes (bench.py, tools/prove_ivc.py); the proofs are the same
            if (chains > 1 && !getenv("VPBS_WIDE_THRESHOLD")) (void)vpbs_ctx_set_option(w.ctx, VPBS_OPT_WIDE_THRESHOLD, 2048);
            rc = vpbs_ivc_create(w.ctx, cyclic, dummy, N, K, ggsw_len, nullptr, &w.ivc, e, sizeof e);
            if (rc != VPBS_OK) return report(err, err_len, std::string("vpbs_ivc_create: ") + e), rc;
            rc = vpbs_ivc_set_device_witness(w.ivc, prm->ELL, prm->LOGB, witness_batch, 0);
            if (rc != VPBS_OK) return report(err, err_len, std::string("vpbs_ivc_set_device_witness: ") + vpbs_ivc_last_error(w.ivc)), rc;
            (void)vpbs_ivc_set_checkpoint(w.ivc, 0, nullptr, nullptr);
        }
        ivc_shape(workers[0].ivc, &shape);
        max_bytes = 8 * (shape.proof_words + shape.n_pi) + (1 << 16);
        return VPBS_OK;
    }
    u64* alloc(size_t words) {
        u64* d = boot_ctx->alloc_words(std::max<size_t>(1, words));
        owned.push_back(d);
        return d;
    }
    // the constants of every step and the workers' buffers, queued on boot_ctx's stream (the caller waits); throws DeviceError
    void alloc_buffers() {
        const IvcShape& sh = shape;
        hipStream_t s = boot_ctx->stream;
        std::vector<u64> consts(sh.cyc_vk, sh.cyc_vk + sh.vk_words);   // own verifier data | dummy verifier data | the dummy proof
        consts.insert(consts.end(), sh.dum_vk, sh.dum_vk + sh.vk_words);
        consts.insert(consts.end(), sh.dummy_proof, sh.dummy_proof + sh.proof_words);
        d_consts = alloc(consts.size());
        VPBS_HIP(hipMemcpyAsync(d_consts, consts.data(), 8 * consts.size(), hipMemcpyHostToDevice, s));
        for (auto& w : workers) {
            w.d_accs = alloc((size_t)total * sh.kn);
            w.d_lwe_links = alloc(4 * (size_t)total);
            w.d_ct = alloc(n_lwe + 1);
            w.d_testv = alloc(sh.N);
            w.d_acc_in = alloc(sh.kn);
            if (!(w.accs = static_cast<u64*>(vpbs_host_alloc(8 * (size_t)total * sh.kn)))) throw DeviceError{VPBS_ERR_OOM, "out of pinned memory"};
            w.lwe_links.resize(4 * (size_t)total);
            w.proof.resize(max_bytes);
        }
        VPBS_HIP(vpbs::stream_sync(s));   // `consts` goes away
    }
    // before the owner destroys boot_ctx
    void destroy() {
        for (auto& w : workers) {
            if (w.accs) vpbs_host_free(w.accs);
            if (w.ivc) vpbs_ivc_free(w.ivc);
            if (w.ctx) vpbs_ctx_destroy(w.ctx);
        }
        workers.clear();
        if (boot_ctx) {
            (void)hipSetDevice(boot_ctx->device);
            (void)vpbs::stream_sync(boot_ctx->stream);
            for (u64* d : owned) boot_ctx->release(d);
        }
        owned.clear();
    }
    PresetArgs preset_args(const Worker& w, unsigned first, unsigned cnt, u64* d_matrix) const {
        PresetArgs a{};
        a.m = d_matrix;
        a.testv = w.d_testv; a.accs = w.d_accs; a.key_links = w.keys.d_key_links; a.lwe_links = w.d_lwe_links; a.ct = w.d_ct;
        a.bsk = w.keys.d_bsk; a.ksk = w.keys.d_ksk; a.consts = d_consts;
        a.first = first; a.cnt = cnt; a.n_lwe = n_lwe; a.N = shape.N;
        a.kn = shape.kn; a.proof_words = shape.proof_words; a.n_pi = shape.n_pi; a.ggsw_len = shape.ggsw_len; a.vk_words = shape.vk_words;
        return a;
    }
    // the chain's public inputs where ivc_prove_pbs_resident wants them: accumulators on the device (the key source, this worker's buffer) and
    // on the host (one copy of (n + 2) K N words), the LWE hash chain on both.  Under boot_mu, on the bootstrap context's stream.
    // from > 0: a resumed chain; acc_from [K N] (host) is the accumulator after step from - 1, and only entries from - 1 .. n + 1 of the
    // accumulators are made and copied.  The LWE links are walked from 0 all the same (730 permutations).
    int prepare_chain(Worker& w, const u64* ct, const u64* testv, std::string& why, unsigned from = 0, const u64* acc_from = nullptr) {
        const size_t kn = shape.kn;
        w.keys = keys_of(w.index);
        u64 in[5] = {0, 0, 0, 0, 0}, h[4];   // verify_hash_output's chain: h_s = hash_no_pad(h_{s-1} || mask_s), masks ct[n], ct[0] .. ct[n-1], 0
        for (unsigned s = 0; s < total; ++s) {
            in[4] = s == 0 ? ct[n_lwe] : (s <= n_lwe ? ct[s - 1] : 0);
            vpbs_hash_no_pad(in, 5, h);
            std::memcpy(in, h, 32);
            std::memcpy(w.lwe_links.data() + 4 * (size_t)s, h, 32);
        }
        std::lock_guard<std::mutex> lk(boot_mu);
        try {
            VPBS_HIP(hipSetDevice(device));
            hipStream_t s = boot_ctx->stream;
            VPBS_HIP(hipMemcpyAsync(w.d_ct, ct, 8 * (size_t)(n_lwe + 1), hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(w.d_testv, testv, 8 * (size_t)shape.N, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(w.d_lwe_links, w.lwe_links.data(), 8 * w.lwe_links.size(), hipMemcpyHostToDevice, s));
            if (from) VPBS_HIP(hipMemcpyAsync(w.d_acc_in, acc_from, 8 * kn, hipMemcpyHostToDevice, s));
            std::string what;
            if (!accumulators(w, from, what)) throw DeviceError{VPBS_ERR_DEVICE, "accumulators of the chain: " + what};
            const size_t lo = from ? from - 1 : 0;   // the first entry this chain reads
            VPBS_HIP(hipMemcpyAsync(w.accs + lo * kn, w.d_accs + lo * kn, 8 * ((size_t)total - lo) * kn, hipMemcpyDeviceToHost, s));
            VPBS_HIP(vpbs::stream_sync(s));
            return VPBS_OK;
        } catch (const DeviceError& e) {
            (void)vpbs::stream_sync(boot_ctx->stream);
            why = e.what;
            return e.status;
        }
    }
    static int fill(void* user, void* stream, unsigned first, unsigned cnt, uint64_t* d_matrix) {
        auto* w = static_cast<Worker*>(user);
        launch_preset(static_cast<hipStream_t>(stream), w->pool->preset_args(*w, first, cnt, d_matrix));
        return hipGetLastError() == hipSuccess ? VPBS_OK : VPBS_ERR_DEVICE;
    }
    static void on_checkpoint(void* user, unsigned done, const uint8_t* bytes, size_t len) {
        auto* w = static_cast<Worker*>(user);
        std::lock_guard<std::mutex> lk(w->pool->cb_mu);
        if (w->pool->ckpt_fn) w->pool->ckpt_fn(w->pool->ckpt_user, w->index, done, bytes, len);
    }
    // ---- what the owners' entry points of the same names do, under the owner's run mutex where they change something ----
    int set_check_witness(int on) {
        for (auto& w : workers) {
            const int rc = vpbs_ivc_set_check_witness(w.ivc, on);
            if (rc != VPBS_OK) return rc;
        }
        return VPBS_OK;
    }
    void witness_checks(uint64_t out[2]) const {
        out[0] = out[1] = 0;
        for (const auto& w : workers) {
            uint64_t c[2] = {0, 0};
            (void)vpbs_ivc_witness_checks(w.ivc, c);
            out[0] += c[0];
            out[1] += c[1];
        }
    }
    void set_checkpoint(unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
        ckpt_fn = every ? fn : nullptr;
        ckpt_user = user;
        for (auto& w : workers) (void)vpbs_ivc_set_checkpoint(w.ivc, fn ? every : 0, fn ? &ProvePool::on_checkpoint : nullptr, &w);
    }
    // The checkpoints of a resume, validated on the host before anything is queued, the rows spread over the worker threads (each uses its
    // own chain's vpbs_ivc, read-only): ivc_open_checkpoint (the prefix form of verify_pbs against the object's own verifier data, LWE hash
    // chain included), the counter against `steps`, then the key hash against link k - 1 of the row's resident key set -- one 32-byte
    // compare; no key chain is walked.  keys_of must answer for the run already.
    void open_checkpoints(const u64* cts, size_t count, const u64* testv, int testv_per_ct, const uint8_t* const* checkpoints, const size_t* lens,
                          unsigned steps, Resume& rs) {
        const unsigned last = steps == 0 || steps > total ? total : steps;
        rs.bytes = checkpoints;
        rs.lens = lens;
        rs.opened.assign(count, IvcCheckpoint{});
        rs.refused.assign(count, std::string());
        rs.resumed = 0;
        if (!checkpoints) return;
        std::vector<size_t> rows;
        for (size_t i = 0; i < count; ++i)
            if (checkpoints[i]) rows.push_back(i);
        const size_t n_threads = std::min(rows.size(), workers.size());
        auto work = [&](size_t t) {
            (void)pthread_setname_np(pthread_self(), "vpbs-ckpt");
            for (size_t r = t; r < rows.size(); r += n_threads) {
                const size_t i = rows[r];
                IvcCheckpoint& cp = rs.opened[i];
                std::string why;
                if (!ivc_open_checkpoint(workers[t].ivc, testv + (testv_per_ct ? i * shape.N : 0), cts + i * (n_lwe + 1), n_lwe, checkpoints[i],
                                         lens ? lens[i] : 0, &cp, &why)) {
                    rs.refused[i] = "checkpoint: " + why;
                } else if (cp.k > last) {
                    rs.refused[i] = "checkpoint: its counter " + std::to_string(cp.k) + " is beyond the requested " + std::to_string(last) + " steps";
                } else if (std::memcmp(cp.pis.data() + 2 * shape.kn + 1, keys_of(i).key_links + 4 * (size_t)(cp.k - 1), 32) != 0) {
                    rs.refused[i] = "checkpoint: the key hash chain does not match";
                }
                if (!rs.refused[i].empty()) cp = IvcCheckpoint{};   // the row starts at step 0 for its outputs and is not proven
            }
        };
        std::vector<std::thread> threads;
        for (size_t t = 0; t < n_threads; ++t) threads.emplace_back(work, t);
        for (auto& t : threads) t.join();
        for (size_t i = 0; i < count; ++i) rs.resumed += rs.opened[i].k != 0;
    }
    // start [c] and acc_in [c][K N] of the rows i0 .. i0 + c of a resume for a run_from launch; false when none of them is resumed
    bool start_rows(const Resume& rs, size_t i0, size_t c, std::vector<uint32_t>& start, std::vector<u64>& acc_in) const {
        bool any = false;
        start.assign(c, 0);
        for (size_t i = 0; i < c; ++i)
            if ((start[i] = rs.opened[i0 + i].k) != 0) any = true;
        if (!any) return false;
        acc_in.resize(c * shape.kn);   // rows that start at 0 are not read
        for (size_t i = 0; i < c; ++i)
            if (start[i]) std::memcpy(acc_in.data() + i * shape.kn, rs.acc_of(i0 + i, shape.kn), 8 * shape.kn);
        return true;
    }
    // the proofs of a run whose outputs are complete (stats.outputs_seconds is set; t_call: when the owner's run began): workers take
    // ciphertext indices from a queue; one that fails reports and takes the next, nobody waits for anybody.  Returns the proofs delivered.
    // rs (a resume): a refused row reports its message and is not proven; an accepted one goes on at its checkpoint's step.
    long prove(const u64* cts, size_t count, const u64* testv, int testv_per_ct, unsigned steps, double t_call, vpbs_pbs_proof_fn proof_fn,
               void* user, const Resume* rs = nullptr) {
        const unsigned last = steps == 0 || steps > total ? total : steps;
        const unsigned N = shape.N;
        const size_t ct_words = n_lwe + 1;
        std::mutex q_mu;
        size_t next = 0;
        long delivered = 0;
        double prepare_s = 0;
        vpbs_ivc_timing sum{};   // over the delivered chains (under cb_mu)
        auto work = [&](Worker& w) {
            (void)pthread_setname_np(pthread_self(), "vpbs-chain");
            for (;;) {
                {
                    std::lock_guard<std::mutex> lk(q_mu);
                    if (next >= count) return;
                    w.index = next++;
                }
                const u64 *ct = cts + w.index * ct_words, *tv = testv + (testv_per_ct ? w.index * N : 0);
                if (rs && !rs->refused[w.index].empty()) {   // exactly once, and nothing queued for the row
                    std::lock_guard<std::mutex> lk(cb_mu);
                    proof_fn(user, w.index, nullptr, 0, rs->refused[w.index].c_str());
                    continue;
                }
                const IvcCheckpoint* cp = rs && rs->opened[w.index].k ? &rs->opened[w.index] : nullptr;
                const unsigned from = cp ? cp->k : 0;
                std::string why;
                const uint8_t* bytes = w.proof.data();
                long n = VPBS_OK;
                double d_prepare = 0;
                vpbs_ivc_timing t{};
                if (cp && from == last) {   // nothing to prove: the validated checkpoint itself
                    bytes = rs->bytes[w.index];
                    n = (long)rs->lens[w.index];
                } else {
                    const double t_prepare = now_s();
                    n = prepare_chain(w, ct, tv, why, from, cp ? rs->acc_of(w.index, shape.kn) : nullptr);
                    d_prepare = now_s() - t_prepare;
                    if (n == VPBS_OK) {
                        const IvcResidentChain chain{w.accs, w.keys.key_links, w.lwe_links.data(), &ProvePool::fill, &w};
                        char e[512] = {0};
                        n = ivc_prove_pbs_resident(w.ivc, tv, ct, n_lwe, &chain, from, cp ? cp->proof.data() : nullptr, cp ? cp->pis.data() : nullptr,
                                                   steps, w.proof.data(), w.proof.size(), &t, e, sizeof e);
                        if (n <= 0) why = e;
                    }
                }
                std::lock_guard<std::mutex> lk(cb_mu);
                if (n > 0) {
                    proof_fn(user, w.index, bytes, (size_t)n, nullptr);
                    ++delivered;
                    prepare_s += d_prepare;
                    sum.seconds += t.seconds; sum.steps = t.steps; sum.base_proof_ms += t.base_proof_ms; sum.late_witness_ms += t.late_witness_ms;
                    sum.late_rows_upload_ms += t.late_rows_upload_ms; sum.prove_step_ms += t.prove_step_ms; sum.early_witness_ms += t.early_witness_ms;
                    sum.late_ahead_ms += t.late_ahead_ms;
                } else {
                    proof_fn(user, w.index, nullptr, 0, why.empty() ? "the chain failed" : why.c_str());
                }
            }
        };
        std::vector<std::thread> threads;
        const size_t n_threads = std::min(count, workers.size());
        for (size_t t = 0; t < n_threads; ++t) threads.emplace_back(work, std::ref(workers[t]));
        for (auto& t : threads) t.join();
        stats.seconds = now_s() - t_call;
        stats.proofs = (size_t)delivered;
        if (delivered) {
            const double d = (double)delivered;
            stats.prepare_chain_ms = 1e3 * prepare_s / d;
            stats.chain = vpbs_ivc_timing{sum.seconds / d, sum.steps, sum.base_proof_ms / d, sum.late_witness_ms / d, sum.late_rows_upload_ms / d,
                                          sum.prove_step_ms / d, sum.early_witness_ms / d, sum.late_ahead_ms / d};
        }
        return delivered;
    }
};
}  // namespace
}  // namespace vpbs

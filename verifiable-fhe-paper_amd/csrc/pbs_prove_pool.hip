// The worker pool of the batch provers (pbs_prove_pool.h): the two kernels that assemble a preset matrix on the device and their launch, the
// chains and their queue, and everything vpbs_pbs_prover (pbs_prove_batch.hip) and vpbs_ring_prover (pbs_prove_ring.hip) do alike --
// creation, the run behind run and resume, the entry points that only pass through.  The library is built without relocatable device code:
// this is the one file that compiles the kernels, and the owners reach them through launch_preset.
#include "pbs_prove_pool.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <pthread.h>
#include <thread>

namespace vpbs {
namespace {
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

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the callbacks a chain's vpbs_ivc takes, user = its worker
int fill(void* user, void* stream, unsigned first, unsigned cnt, uint64_t* d_matrix) {
    auto* w = static_cast<ProvePool::Worker*>(user);
    launch_preset(static_cast<hipStream_t>(stream), w->pool->preset_args(*w, first, cnt, d_matrix));
    return hipGetLastError() == hipSuccess ? VPBS_OK : VPBS_ERR_DEVICE;
}
void on_checkpoint(void* user, unsigned done, const uint8_t* bytes, size_t len) {
    auto* w = static_cast<ProvePool::Worker*>(user);
    std::lock_guard<std::mutex> lk(w->pool->cb_mu);
    if (w->pool->ckpt_fn) w->pool->ckpt_fn(w->pool->ckpt_user, w->index, done, bytes, len);
}
}  // namespace

void launch_preset(hipStream_t s, const PresetArgs& a) {
    const size_t words = a.plain_rows() * a.cnt;
    hipLaunchKernelGGL(preset_rows_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a);
    const size_t longer = std::max(a.ggsw_len, a.kn);
    hipLaunchKernelGGL(preset_transpose_kernel, dim3((unsigned)((longer + TILE_K - 1) / TILE_K), (a.cnt + TILE_I - 1) / TILE_I, 2), dim3(256), 0, s, a);
}

int ProvePool::create(int device_ordinal, const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, const vpbs_tfhe_params* prm, unsigned n,
                      unsigned chains, unsigned witness_batch, char* err, size_t err_len, const std::function<int()>& before_chains) {
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!cyclic || !dummy || !prm || !cyclic->circuit || !dummy->circuit) return refuse("null argument");
    if (chains == 0 || chains > 64) return refuse("chains must be 1 .. 64");
    if (witness_batch == 0) return refuse("witness_batch must be at least 1 (the batch prover runs the device-witness pipeline)");
    if (prm->log_N < 1 || prm->log_N > 11 || prm->K < 2 || prm->ELL < 1 || prm->LOGB < 1) return refuse("unsupported TFHE parameters");
    if (n == 0) return refuse("n_lwe must be at least 1");
    device = device_ordinal;
    n_lwe = n;
    total = n + 2;
    const unsigned N = 1u << prm->log_N, K = prm->K;
    const size_t ggsw_len = (size_t)K * prm->ELL * K * N;
    const unsigned log_n_max = std::max(16u, cyclic->circuit->log_n);
    int rc = vpbs_ctx_create(device, log_n_max, 3, 4, &boot_ctx);
    if (rc != VPBS_OK) return report(err, err_len, "the bootstrap context could not be made (no such device?)"), rc;
    if (before_chains && (rc = before_chains()) != VPBS_OK) return rc;
    char e[512] = {0};
    workers.resize(chains);
    for (auto& w : workers) {
        w.pool = this;
        rc = vpbs_ctx_create(device, log_n_max, 3, 4, &w.ctx);
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

int ProvePool::alloc_buffers(char* err, size_t err_len) {
    const IvcShape& sh = shape;
    hipStream_t s = boot_ctx->stream;
    try {
        VPBS_HIP(hipSetDevice(device));
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
        return VPBS_OK;
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(s);
        report(err, err_len, x.what);
        return x.status;
    }
}

void ProvePool::destroy() {
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

ProvePool::~ProvePool() {
    destroy();
    if (boot_ctx) vpbs_ctx_destroy(boot_ctx);
}

PresetArgs ProvePool::preset_args(const Worker& w, unsigned first, unsigned cnt, u64* d_matrix) const {
    PresetArgs a{};
    a.m = d_matrix;
    a.testv = w.d_testv; a.accs = w.d_accs; a.key_links = w.keys.d_key_links; a.lwe_links = w.d_lwe_links; a.ct = w.d_ct;
    a.bsk = w.keys.d_bsk; a.ksk = w.keys.d_ksk; a.consts = d_consts;
    a.first = first; a.cnt = cnt; a.n_lwe = n_lwe; a.N = shape.N;
    a.kn = shape.kn; a.proof_words = shape.proof_words; a.n_pi = shape.n_pi; a.ggsw_len = shape.ggsw_len; a.vk_words = shape.vk_words;
    return a;
}

int ProvePool::prepare_chain(Worker& w, const u64* ct, const u64* testv, std::string& why, unsigned from, const u64* acc_from) {
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

void ProvePool::open_checkpoints(const u64* cts, size_t count, const u64* testv, int testv_per_ct, const uint8_t* const* checkpoints,
                                 const size_t* lens, unsigned steps, Resume& rs) {
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

bool ProvePool::start_rows(const Resume& rs, size_t i0, size_t c, std::vector<uint32_t>& start, std::vector<u64>& acc_in) const {
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

long ProvePool::prove(const u64* cts, size_t count, const u64* testv, int testv_per_ct, unsigned steps, double t_call, vpbs_pbs_proof_fn proof_fn,
                      void* user, const Resume* rs) {
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
                    const IvcResidentChain chain{w.accs, w.keys.key_links, w.lwe_links.data(), &fill, &w};
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

long ProvePool::check_run(PoolRef r, const u64* cts, size_t count, const u64* testv, const uint32_t* const* key_of,
                          const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, vpbs_pbs_proof_fn proof_fn, char* err, size_t err_len) {
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!proof_fn) return refuse("no proof_fn: the proofs have nowhere to go");
    if (count && (!cts || !testv || (key_of && !*key_of))) return refuse(key_of ? "null cts, testv or key_of" : "null cts or testv");
    if (count && checkpoints && !lens) return refuse("checkpoints without lens");
    if (!r.pool) return refuse("null prover");
    if (steps > r.pool->total) return refuse("steps exceeds n_lwe + 2 = " + std::to_string(r.pool->total));
    return count != 0;
}

long ProvePool::run(const u64* cts, size_t count, const u64* testv, int testv_per_ct, const uint8_t* const* checkpoints, const size_t* lens,
                    unsigned steps, u64* out_ct, u64* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    const double t_call = now_s();
    stats = vpbs_pbs_run_stats{};
    const size_t kn = shape.kn, ct_words = n_lwe + 1;
    // ---- a resume: every checkpoint validated on the host before anything is queued, its key hash against the links of the row's key set ----
    Resume rs;
    if (checkpoints) open_checkpoints(cts, count, testv, testv_per_ct, checkpoints, lens, steps, rs);
    // ---- every output first: one launch of the key source per OUT_BATCH ciphertexts; accepted rows enter at their checkpoint's step ----
    if (out_ct || lwe_out) {
        std::lock_guard<std::mutex> lk(boot_mu);
        std::vector<uint32_t> start;
        std::vector<u64> acc_in;
        for (size_t i0 = 0; i0 < count; i0 += OUT_BATCH) {
            const size_t c = std::min(OUT_BATCH, count - i0);
            const bool from = rs.resumed && start_rows(rs, i0, c, start, acc_in);
            const long rc = outputs(i0, c, cts + i0 * ct_words, from ? start.data() : nullptr, from ? acc_in.data() : nullptr,
                                    testv + (testv_per_ct ? i0 * shape.N : 0), testv_per_ct, out_ct ? out_ct + i0 * kn : nullptr,
                                    lwe_out ? lwe_out + i0 * ct_words : nullptr);
            if (rc != (long)c) {
                report(err, err_len, std::string(outputs_name) + (from ? "_from: " : ": ") + vpbs_last_error(boot_ctx));
                return rc < 0 ? rc : (long)VPBS_ERR_DEVICE;
            }
        }
    }
    // ---- the proofs: the workers take ciphertext indices from a queue; each chain under the keys and links of its key set ----
    stats.outputs_seconds = out_ct || lwe_out ? now_s() - t_call : 0.0;
    return prove(cts, count, testv, testv_per_ct, steps, t_call, proof_fn, user, checkpoints ? &rs : nullptr);
}

int ProvePool::verifier_data(PoolRef r, uint64_t* cyclic_vk, uint64_t* dummy_vk) {
    if (!r.pool) return VPBS_ERR_INVALID;
    return vpbs_ivc_verifier_data(r.pool->workers[0].ivc, cyclic_vk, dummy_vk);
}

int ProvePool::set_check_witness(PoolRef r, int on) {
    if (!r.pool) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(*r.run_mu);
    for (auto& w : r.pool->workers) {
        const int rc = vpbs_ivc_set_check_witness(w.ivc, on);
        if (rc != VPBS_OK) return rc;
    }
    return VPBS_OK;
}

int ProvePool::witness_checks(PoolRef r, uint64_t out[2]) {
    if (!r.pool || !out) return VPBS_ERR_INVALID;
    out[0] = out[1] = 0;
    for (const auto& w : r.pool->workers) {
        uint64_t c[2] = {0, 0};
        (void)vpbs_ivc_witness_checks(w.ivc, c);
        out[0] += c[0];
        out[1] += c[1];
    }
    return VPBS_OK;
}

int ProvePool::set_checkpoint(PoolRef r, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
    if (!r.pool) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(*r.run_mu);
    r.pool->ckpt_fn = every ? fn : nullptr;
    r.pool->ckpt_user = user;
    for (auto& w : r.pool->workers) (void)vpbs_ivc_set_checkpoint(w.ivc, fn ? every : 0, fn ? &on_checkpoint : nullptr, &w);
    return VPBS_OK;
}

int ProvePool::last_run(PoolRef r, vpbs_pbs_run_stats* out) {
    if (!r.pool || !out) return VPBS_ERR_INVALID;
    *out = r.pool->stats;
    return VPBS_OK;
}
}  // namespace vpbs

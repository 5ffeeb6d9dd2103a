// One verifiable PBS as the reference produces it, as ONE call: the IVC chain of `verified_pbs`
// (/root/reference/src/vtfhe/ivc_based_vpbs.rs:159-386: build the cyclic step circuit, prove the base case, then n + 2 steps each verifying its
// predecessor in circuit) driven inside the library.  Host code only, written against the library's own C ABI (include/vpbs_prover.h) -- what
// examples/prove_ivc.cpp did by hand: nothing here reaches below that boundary.
//   create : (comm != NULL: coset-sharded over the GPUs of a node -- every rank calls with its own context and communicator, generates the
//            same witnesses, proves its cosets of every step and ends with the same proof)
//            constants/sigmas commitments and verifier data of the cyclic and the dummy circuit (CircuitBuilder::build's prover data),
//            compiled witness plans, the split of the cyclic plan (the previous proof's words are the late part), three pinned + three
//            device wire matrices
//   prove  : ONE loop (ChainRun) on the calling thread: base proof of the dummy circuit (cyclic_base_proof, :292-299), then per step the
//            late witness phase (the previous proof's words: vpbs_witness_plan_run_late_packed), the scatter of its values into the
//            step's device matrix, vpbs_prove_step, the step hook and the checkpoint; the last proof serialised
//            (ProofWithPublicInputs::to_bytes).  Who STAGES a step -- its device matrix with the early wires, its public inputs, its late
//            state -- is a StepSource, and there are two:
//              host pipeline (prove_pbs_host, the default)
//                thread E  vpbs_witness_plan_run_early   everything that does not need the previous proof; yields the step's public inputs
//                thread U  vpbs_device_upload_bg         that matrix to the device while the previous step is being proven
//              device pipeline (prove_pbs_device_witness, vpbs_ivc_set_device_witness)
//                the public inputs of ALL steps natively (accumulator chain; thread H walks the two hash chains), then
//                thread B  vpbs_witness_device_run       the early phases of a batch of steps on one of two device objects
//                thread S  vpbs_witness_device_wires     a step's wires into a device matrix, its late state seeded from the device
//                (late phase on the device: no thread S, the loop runs vpbs_witness_device_run_late itself; resident chain: the public
//                inputs are given, ivc_resident.h)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <pthread.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vpbs_prover.h"
#include "ivc_resident.h"
#include "test_entries.h"

// The one thing this driver takes from the library beside the public header: vpbs_device_scatter's copy + kernel QUEUED on the context's
// stream without the wait (api.hip).  A host that writes its own loop over the C ABI calls vpbs_device_scatter and pays the wait.
namespace vpbs {
int device_scatter(vpbs_ctx* c, uint64_t* d_dst, const uint64_t* d_positions, const uint64_t* host_values, size_t count, uint64_t* d_stage, bool wait);
// ... and the late witness phase on the device stage by stage (witness_device.hip): queued as the previous proof's sections become final
unsigned witness_device_late_stages(const vpbs_witness_device* d);
int witness_device_run_late_stage(vpbs_witness_device* d, unsigned instance, unsigned stage, const uint64_t* preset_val, int wait);
// ... the accumulator chain from a later step (api.hip) and the two halves of vpbs_verify_pbs_prefix (verifier.hip), for vpbs_ivc_resume_pbs
int pbs_accumulator_chain_from(vpbs_ctx* c, const vpbs_tfhe_params* prm, unsigned n_lwe, unsigned start, const uint64_t* acc_in,
                               const uint64_t* lwe_ct, const uint64_t* bsk, const uint64_t* ksk, uint64_t* accs_out);
int verify_pbs_prefix_without_keys(const vpbs_verify_pbs_inputs* in, const uint8_t* bytes, size_t len, unsigned* steps_done, char* why, size_t why_len);
bool pbs_key_chain_prefix_matches(const vpbs_verify_pbs_inputs* in, unsigned k, const uint64_t claimed[4]);
}

namespace {
using u64 = uint64_t;

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the role of a thread in /proc/<pid>/task/*/comm: CPU time by role is how a host sizes a rank's CPU share (tools/prove_ivc.py VPBS_CPU_BY_ROLE)
void name_thread(const char* name) { (void)pthread_setname_np(pthread_self(), name); }
// CPU seconds the CALLING thread has used (VPBS_TRACE_IVC: what the proving thread burns while it waits for the device)
double thread_cpu() {
    timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? ts.tv_sec + 1e-9 * ts.tv_nsec : 0.0;
}
// the message of an entry point into the caller's buffer (none: dropped)
void report(char* err, size_t err_len, const std::string& m) {
    if (err && err_len) {
        std::strncpy(err, m.c_str(), err_len - 1);
        err[err_len - 1] = 0;
    }
}
// steps = 0, or more than the chain has: the whole chain of n + 2 steps
unsigned clamp_steps(unsigned steps, unsigned n_lwe) { return steps == 0 || steps > n_lwe + 2 ? n_lwe + 2 : steps; }
// the one owner of a late state (vpbs_witness_plan_run_early / vpbs_witness_state_from_late_inputs make it, run_late consumes it): a
// failure on the way must not leak tens of MB of slot values
struct StateFree {
    void operator()(vpbs_witness_state* s) const { vpbs_witness_state_free(s); }
};
using State = std::unique_ptr<vpbs_witness_state, StateFree>;

struct Side {   // one circuit on the context
    vpbs_ctx* ctx = nullptr;
    unsigned log_n = 0, n_wires = 0, n_routed = 0, n_const_cols = 0, num_selectors = 0;
    size_t n = 0;
    std::vector<vpbs_gate> gates;
    std::vector<uint32_t> pi_pos;   // cyclic circuit only (the dummy circuit's public inputs are its PartialWitness, never read back)
    size_t n_pi = 0, n_preset = 0;
    std::vector<u64> cs_cap, vk;   // vk: circuit digest [4] then the constants/sigmas cap
    u64* d_sigma = nullptr;
    u64* d_csv = nullptr;          // sharded commitment only: the constants / sigmas matrix on the device
    vpbs_batch* cs = nullptr;
    vpbs_witness_plan* plan = nullptr;
    const vpbs_comm* comm = nullptr;   // not null: every commitment and proof of this circuit is coset-sharded over comm->world GPUs
    // the witness check (vpbs_ivc_set_check_witness): the circuit's tables are kept on the host so that a checker can be made later
    std::vector<uint32_t> row_gate, copies;
    std::vector<u64> constants;
    vpbs_witness_checker* chk = nullptr;
    u64* checks = nullptr;             // {witnesses checked, violations}, the chain's counters

    int init(vpbs_ctx* c, const vpbs_ivc_circuit& d, unsigned cap_height, const vpbs_comm* cm, std::string& err) {
        ctx = c;
        comm = cm;
        const vpbs_circuit& k = *d.circuit;
        log_n = k.log_n; n_wires = k.n_wires; n_routed = k.n_routed; n_const_cols = k.n_constants_cols; num_selectors = k.num_selectors;
        n = (size_t)1 << log_n;
        gates.assign(k.gates, k.gates + k.n_gates);
        row_gate.assign(k.row_gate, k.row_gate + n);
        copies.assign(k.copies, k.copies + 2 * k.n_copies);
        constants.assign(k.constants, k.constants + (size_t)n_const_cols * n);
        if (d.pi_pos) pi_pos.assign(d.pi_pos, d.pi_pos + d.n_pi);
        n_pi = d.n_pi;
        n_preset = d.n_preset;
        std::vector<u64> csv((size_t)(n_const_cols + n_routed) * n);
        std::memcpy(csv.data(), k.constants, 8 * (size_t)n_const_cols * n);
        u64* sigma = csv.data() + (size_t)n_const_cols * n;
        if (vpbs_sigma_values(&k, sigma) != 0) return err = "sigma polynomials: malformed copy constraints", VPBS_ERR_INVALID;
        const size_t cap_words = (size_t)4 << cap_height;
        cs_cap.resize(cap_words);
        int rc;
        if (!comm) {
            rc = vpbs_commit_values(ctx, csv.data(), n_const_cols + n_routed, log_n, &cs, cs_cap.data());
        } else {   // this rank's cosets; the cap is the concatenation of every rank's part (one all-gather of 32-byte hashes)
            if (comm->world == 0 || cap_words % comm->world != 0 || !comm->allgather) return err = "malformed communicator", VPBS_ERR_INVALID;
            rc = vpbs_device_alloc(ctx, csv.size(), &d_csv);
            if (rc == 0) rc = vpbs_device_upload(ctx, d_csv, csv.data(), csv.size());
            std::vector<u64> local(cap_words / comm->world);
            if (rc == 0) rc = vpbs_commit_sharded_dev(ctx, d_csv, 1, n_const_cols + n_routed, log_n, comm->rank, comm->world, &cs, local.data());
            // the all-gather carries every rank's status: a rank whose commitment failed still takes part, and all ranks return an error
            const int own = rc;
            rc = vpbs_comm_allgather_checked(comm, local.data(), local.size(), cs_cap.data(), own);
            if (rc != 0 && own == 0)
                return err = rc == VPBS_ERR_PEER ? "constants / sigmas commitment: another rank failed" : "all-gather of the cap failed", rc;
        }
        if (rc != 0) return err = std::string("constants / sigmas commitment: ") + vpbs_last_error(ctx), rc;
        vk.assign(4, 0);
        vpbs_compat compat;
        vpbs_ctx_get_compat(ctx, &compat);
        vpbs_circuit_digest(&compat, cs_cap.data(), cs_cap.size(), log_n, vk.data());   // CircuitBuilder::build's circuit_digest
        vk.insert(vk.end(), cs_cap.begin(), cs_cap.end());
        rc = vpbs_device_alloc(ctx, (size_t)n_routed * n, &d_sigma);
        if (rc == 0) rc = vpbs_device_upload(ctx, d_sigma, sigma, (size_t)n_routed * n);
        if (rc != 0) return err = std::string("sigma values to the device: ") + vpbs_last_error(ctx), rc;
        char e[256] = {0};
        rc = vpbs_witness_plan_create(&k, d.preset_pos, d.n_preset, &plan, e, sizeof e);
        if (rc != 0) return err = std::string("witness plan: ") + e, rc;
        return VPBS_OK;
    }
    void step_inputs(vpbs_step_inputs& in, const u64* wires, bool on_device, const u64* pis) const {
        in = vpbs_step_inputs{};
        in.log_n = log_n; in.n_wires = n_wires; in.n_zs_partial_products = 20; in.n_quotient = 16; in.num_challenges = 2;
        in.inputs_on_device = on_device ? 1 : 0;
        in.wires_values = wires;
        in.constants_sigmas = cs;
        for (int i = 0; i < 4; ++i) in.circuit_digest[i] = vk[i];
        in.public_inputs = pis; in.n_public_inputs = n_pi;
        in.forced_pow = VPBS_POW_ANY;
        in.sigmas_values = d_sigma; in.sigmas_on_device = 1;
        in.n_routed = n_routed; in.quotient_degree_factor = 8; in.n_constants = n_const_cols;
        in.gates = gates.data(); in.n_gates = (unsigned)gates.size(); in.num_selectors = num_selectors;
    }
    int prove(const vpbs_step_inputs& in, u64* caps, u64* openings, u64* fri) const {
        if (chk) {   // never sharded (vpbs_ivc_set_check_witness refuses a chain with a communicator)
            const int rc = vpbs_prove_step_checked(ctx, chk, &in, caps, openings, fri, nullptr, nullptr);
            if (rc == VPBS_OK || rc == VPBS_ERR_WITNESS) ++checks[0];
            if (rc == VPBS_ERR_WITNESS) ++checks[1];
            return rc;
        }
        return comm ? vpbs_prove_step_sharded(ctx, &in, comm, caps, openings, fri, nullptr, nullptr)
                    : vpbs_prove_step(ctx, &in, caps, openings, fri, nullptr, nullptr);
    }
    // a checker of this circuit on the context (on) or none (!on)
    int set_check(bool on, u64* counters, std::string& err) {
        if (chk) vpbs_witness_checker_free(chk);
        chk = nullptr;
        checks = counters;
        if (!on) return VPBS_OK;
        const vpbs_circuit k{log_n, n_wires, n_routed, gates.data(), (unsigned)gates.size(), num_selectors, row_gate.data(), constants.data(),
                             n_const_cols, copies.data(), copies.size() / 2, nullptr, 0};
        char e[256] = {0};
        const int rc = vpbs_witness_checker_create(ctx, &k, &chk, e, sizeof e);
        if (rc != VPBS_OK) err = std::string("witness checker: ") + e;
        return rc;
    }
    void release() {
        if (chk) vpbs_witness_checker_free(chk);
        chk = nullptr;
        if (plan) vpbs_witness_plan_free(plan);
        if (cs) vpbs_batch_free(cs);
        if (d_sigma) vpbs_device_free(ctx, d_sigma);
        if (d_csv) vpbs_device_free(ctx, d_csv);
        plan = nullptr; cs = nullptr; d_sigma = nullptr; d_csv = nullptr;
    }
};
// The late witness phase of step s + 1 in STAGES, started before the proof of step s is complete (the reference's loop
// ivc_based_vpbs.rs:323-353 hands a finished proof to the next step -- here the next step's in-circuit verifier starts on the sections of
// the proof as the prover finishes them).  The proof words are late presets of three stages (vpbs_witness_plan_split with stage numbers):
//   1            caps and openings        -> the in-circuit transcript up to the FRI challenges, the vanishing check at zeta, the reduced openings
//   2 .. 1 + R   the commit cap of FRI round r    -> the transcript absorbs it, the round's folding challenge
//   2 + R        final polynomial, proof-of-work witness -> the rest of the transcript, the query indices
//   3 + R        the query rounds         -> Merkle paths, folds: what is left on the critical path when the proof returns
// (R = 3 reduction rounds at degree 2^16.)  A worker thread runs all but the last on the next step's state (vpbs_witness_plan_run_late_stage) while the previous proof's FRI stage is
// still on the device; vpbs_step_inputs.on_section posts them.  The caller then drains the worker and runs vpbs_witness_plan_run_late_packed,
// which only has stage 3 left.
struct LateAhead {
    const vpbs_witness_plan* plan = nullptr;
    std::vector<std::vector<std::pair<size_t, size_t>>> ranges;   // per stage: [begin, end) word ranges of the flat proof
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    vpbs_witness_state* st = nullptr;   // the job: state and PartialWitness values of the NEXT step, the proof being written
    u64* values = nullptr;
    const u64* proof = nullptr;
    u64* packed = nullptr;              // the pinned buffer of the packed late wires: a stage leaves its share there at once
    unsigned posted = 0, done = 0;
    bool quit = false, failed = false;
    std::string err;
    double busy_s = 0;

    // stage of every proof word -> late mask for vpbs_witness_plan_split (the other presets: 0) and the ranges a stage copies
    void layout(size_t cap_words, size_t openings_words, size_t fri_words, unsigned n_rounds, size_t final_words, std::vector<uint8_t>& late) {
        const size_t head = 3 * cap_words + openings_words, fri_caps = (size_t)n_rounds * cap_words, tail = final_words + 1;
        ranges.assign(n_rounds + 3, {});
        ranges[0].push_back({0, head});                                                                  // section 1
        for (unsigned r = 0; r < n_rounds; ++r) ranges[1 + r].push_back({head + r * cap_words, head + (r + 1) * cap_words});   // sections 2 .. 1 + n_rounds
        ranges[n_rounds + 1].push_back({head + fri_words - tail, head + fri_words});                     // section 2 + n_rounds
        ranges[n_rounds + 2].push_back({head + fri_caps, head + fri_words - tail});                      // the return of the call
        for (size_t k = 0; k < ranges.size(); ++k)
            for (auto& r : ranges[k]) std::fill(late.begin() + r.first, late.begin() + r.second, (uint8_t)(k + 1));
    }
    void start(const vpbs_witness_plan* p) {
        plan = p;
        th = std::thread([this] {
            name_thread("vpbs-late-ahead");
            run();
        });
    }
    bool active() const { return st != nullptr; }
    void begin(vpbs_witness_state* state, u64* vals, const u64* proof_words) {   // proving thread, nothing posted yet
        std::lock_guard<std::mutex> lk(m);
        st = state; values = vals; proof = proof_words;
        posted = done = 0;
        failed = false;
        err.clear();
    }
    void post(unsigned stage) {   // proving thread (on_section): the words of stages <= stage are final
        {
            std::lock_guard<std::mutex> lk(m);
            posted = std::max(posted, std::min<unsigned>(stage, (unsigned)ranges.size() - 1));   // the last stage waits for the return
        }
        cv.notify_all();
    }
    // waits for the posted stages; afterwards the job is the caller's again (run_late for the rest).  false: a stage failed (msg)
    bool drain(std::string& msg) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done >= posted; });
        st = nullptr;
        if (failed) msg = err;
        return !failed;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    ~LateAhead() { stop(); }

  private:
    void run() {
        char e[256];
        for (;;) {
            unsigned stage;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return quit || (st && done < posted); });
                if (quit) return;
                stage = done + 1;
            }
            const double t = now();
            bool ok = !failed;
            if (ok) {
                if (values != proof)
                    for (auto& r : ranges[stage - 1]) std::memcpy(values + r.first, proof + r.first, 8 * (r.second - r.first));
                e[0] = 0;
                ok = vpbs_witness_plan_run_late_stage(plan, st, stage, values, packed, e, sizeof e) == 0;
            }
            {
                std::lock_guard<std::mutex> lk(m);
                busy_s += now() - t;
                if (!ok && !failed) {
                    failed = true;
                    err = e;
                }
                done = stage;
            }
            cv.notify_all();
        }
    }
};
}  // namespace

struct vpbs_ivc {
    vpbs_ctx* ctx = nullptr;
    Side cyc, dum;
    unsigned N = 0, K = 0;
    size_t proof_words = 0, ggsw_len = 0, kn = 0, n_pi = 0, wire_words = 0;
    std::vector<u64> dummy_proof;   // the second proof slot: the dummy circuit's proof of all-zero public inputs (vpbs_ivc_create)
    bool staged = false;            // the cyclic plan is split into late stages by proof section (LateAhead)
    LateAhead ahead_layout;         // ranges only (the worker belongs to a prove_pbs call)
    size_t late_rows[2] = {0, 0};
    size_t late_count = 0;                       // wire positions the late witness phase writes (vpbs_witness_plan_late_count)
    u64 *late_vals = nullptr;                    // their values, packed, pinned (vpbs_witness_plan_run_late_packed)
    u64 *d_late_pos = nullptr, *d_late_stage = nullptr;   // device: the uint32 positions, the staging buffer of vpbs_device_scatter
    static constexpr int NBUF = 3;
    u64 *bufs[NBUF] = {nullptr, nullptr, nullptr}, *d_bufs[NBUF] = {nullptr, nullptr, nullptr}, *base_wires = nullptr;
    bool filled[NBUF] = {false, false, false};
    std::string err;
    vpbs_comm comm{};
    vpbs_ivc_step_fn step_fn = nullptr;
    void* step_user = nullptr;
    vpbs_ivc_checkpoint_fn ckpt_fn = nullptr;   // vpbs_ivc_set_checkpoint
    void* ckpt_user = nullptr;
    unsigned ckpt_every = 0;
    unsigned ckpt_base = 0;   // a resident chain that goes on at step k (ivc_prove_pbs_resident) counts its `every` from k; `done` stays absolute
    std::vector<uint8_t> ckpt_bytes;
    // a step proof of the cyclic circuit as ProofWithPublicInputs::to_bytes writes it: what a call returns and what a checkpoint is
    long to_bytes(const vpbs_step_inputs& in, const u64* caps, const u64* openings, const u64* fri, uint8_t* out, size_t capacity) const {
        return vpbs_step_proof_to_bytes(ctx, &in, cyc.n_const_cols, caps, openings, fri, out, capacity);
    }
    // after chained step `done` of a call that ends at step `last`: the proof serialised exactly as a call with steps = done returns it
    int checkpoint(const vpbs_step_inputs& in, const u64* caps, const u64* openings, const u64* fri, unsigned done, unsigned last) {
        if (!ckpt_fn || !ckpt_every || (done - ckpt_base) % ckpt_every != 0 || done >= last) return VPBS_OK;
        if (ckpt_bytes.empty()) ckpt_bytes.resize(8 * (proof_words + n_pi) + (1 << 16));
        const long n = to_bytes(in, caps, openings, fri, ckpt_bytes.data(), ckpt_bytes.size());
        if (n <= 0) return VPBS_ERR_INVALID;
        ckpt_fn(ckpt_user, done, ckpt_bytes.data(), (size_t)n);
        return VPBS_OK;
    }
    // early witness phases on the device (vpbs_ivc_set_device_witness): two early-only device objects, each on a context of its own (their
    // runs overlap with the prover's context and with each other's gathers), filled alternately with batches of `dw_batch` steps
    unsigned dw_batch = 0, ELL = 0, LOGB = 0;
    bool dw_late = false;   // the late phase on the device too (vpbs_witness_device_run_late): the host generates no witness at all
    vpbs_ctx* wctx[2] = {nullptr, nullptr};
    vpbs_witness_device* wdev[2] = {nullptr, nullptr};
    u64* dw_presets = nullptr;   // pinned [n_preset][dw_batch]
    u64 checks[2] = {0, 0};      // vpbs_ivc_witness_checks
    size_t late_in_count = 0;
    void drop_device_witness() {
        for (int i = 0; i < 2; ++i) {
            if (wdev[i]) vpbs_witness_device_free(wdev[i]);
            if (wctx[i]) vpbs_ctx_destroy(wctx[i]);
            wdev[i] = nullptr;
            wctx[i] = nullptr;
        }
        if (dw_presets) vpbs_host_free(dw_presets);
        dw_presets = nullptr;
        dw_batch = 0;
    }
    ~vpbs_ivc() {
        for (auto b : bufs)
            if (b) vpbs_host_free(b);
        drop_device_witness();
        for (auto d : d_bufs)
            if (d) vpbs_device_free(ctx, d);
        if (base_wires) vpbs_host_free(base_wires);
        if (late_vals) vpbs_host_free(late_vals);
        if (d_late_pos) vpbs_device_free(ctx, d_late_pos);
        if (d_late_stage) vpbs_device_free(ctx, d_late_stage);
        cyc.release();
        dum.release();
    }
};

namespace {
// One call's arguments, as vpbs_ivc_prove_pbs, vpbs_ivc_resume_pbs and vpbs::ivc_prove_pbs_resident pass them on.  from > 0: a resume --
// no base proof, step `from` takes from_proof [proof_words] as its inner proof and from_pis [n_pi] as its predecessor's public inputs.
struct ChainArgs {
    vpbs_ivc* v;
    const u64 *testv, *ct, *bsk, *ksk;
    unsigned n_lwe, from;
    const u64 *from_proof, *from_pis;
    unsigned steps;
    uint8_t* proof_out;
    size_t capacity;
    vpbs_ivc_timing* timing;
    char* err;
    size_t err_len;
};
// One step as a pipeline hands it to the loop: the early wires are in device matrix `buf`, `pis` are the step's public inputs, `state` is
// what the late phase goes on from (none: the late phase runs on the device) and `values` the PartialWitness values that phase reads -- only
// the previous proof's words, at the front.  The host pipeline builds an array per step (own_*); the device pipeline's steps read the loop's.
struct Staged {
    int buf = -1;   // -1: no step
    const u64* pis = nullptr;
    u64* values = nullptr;
    State state;
    std::vector<u64> own_values, own_pis;
};
// What a pipeline is to the loop.  j counts the steps of THIS call: local step j is chain step from + j.
struct StepSource {
    // blocks until step j is staged and its public inputs are complete; fills `step` unless try_take has (buf >= 0).  false: the run failed
    std::function<bool(unsigned j, Staged& step)> take;
    // step j if it is staged by now: asked from inside the previous step's proof (on_section), so it never waits
    std::function<bool(unsigned j, Staged& step)> try_take;
    // step j is proven: its device matrix is free again
    std::function<void(unsigned j, const Staged& step)> release;
    // late phase on the device only: on_section of the proof of step j (DevHook)
    std::function<void(unsigned j, vpbs_step_inputs& in)> arm_device_late;
    // device pipeline only: what take waited for {the staged wires, the hash chain} in seconds, and with them the VPBS_TRACE_IVC line
    const double* waits = nullptr;
};
// The frame of one chain run: what both pipelines own -- arguments, error reporting, the producer threads and the lock they share with the
// loop, the proof buffer, the LateAhead worker, the timers -- and the chain itself, stated once: base(), step() per step, tail().
struct ChainRun : ChainArgs {
    Side &cyc, &dum;
    vpbs_ctx* const ctx;
    const size_t proof_words, ggsw_len;
    const unsigned n_run;
    const std::vector<u64> zero_ggsw;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<bool> failed{false};   // every wait predicate names it
    std::string thread_err;
    std::vector<std::thread> producers;
    // the clock: from here in the device pipeline (its native accumulator chain counts); the host pipeline restarts it at the base proof
    double t0 = now();
    double t_base = 0, t_early = 0, t_late = 0, t_rows = 0, t_prove = 0;   // t_early: the pipeline's (thread E, thread B)
    double c_late = 0, c_rows = 0, c_prove = 0, lap_t = 0, lap_c = 0;      // CPU time of THIS thread in the same sections (VPBS_TRACE_IVC)
    // the previous proof, in the flat order of the proof targets.  A whole PartialWitness array with the proof at its front: the late phase
    // reads the late presets only, so the prover writes straight into what the device pipeline's steps read (Staged::values)
    std::vector<u64> proof;
    u64 *const caps, *openings = nullptr, *fri = nullptr;
    vpbs_step_inputs in;
    char e[256] = {0};
    // The next step's late stages 1 and 2 run on a worker while this step's FRI stage is on the device (LateAhead): the prover reports its
    // sections (on_section, on this thread); the first report that finds the next step staged takes it.  The steps are declared before the
    // worker: the worker is joined before the state it may be working on goes away.
    Staged cur, next;
    LateAhead ahead;
    const StepSource* src = nullptr;
    unsigned j = 0;   // the step being proven

    explicit ChainRun(const ChainArgs& a)
        : ChainArgs(a), cyc(a.v->cyc), dum(a.v->dum), ctx(a.v->ctx), proof_words(a.v->proof_words), ggsw_len(a.v->ggsw_len), n_run(a.steps - a.from),
          zero_ggsw(a.v->ggsw_len, 0), proof(a.v->cyc.n_preset, 0), caps(proof.data()) {}
    void say(const std::string& m) { report(err, err_len, m); }
    // GGSW and mask of chain step s: nothing in the base step, a bootstrapping key and its mask, then the key-switching key
    const u64* ggsw_of(unsigned s) const { return s == 0 ? zero_ggsw.data() : (s <= n_lwe ? bsk + (size_t)(s - 1) * ggsw_len : ksk); }
    u64 mask_of(unsigned s) const { return s == 0 ? ct[n_lwe] : (s <= n_lwe ? ct[s - 1] : (u64)0); }
    void fail(const std::string& m) {
        {   // the flag changes under the lock: a waiter that has just evaluated its predicate cannot miss the notification
            std::lock_guard<std::mutex> lk(mu);
            if (thread_err.empty()) thread_err = m;
            failed = true;
        }
        cv.notify_all();
    }
    void spawn(const char* name, std::function<void()> body) {
        producers.emplace_back([name, body] {
            name_thread(name);
            body();
        });
    }
    void join() {
        for (auto& t : producers)
            if (t.joinable()) t.join();
    }
    // fails, joins every producer and reports the FIRST error of the run
    long stop(const std::string& m, int rc) {
        fail(m);
        join();
        std::string first;
        {
            std::lock_guard<std::mutex> lk(mu);
            first = thread_err;
        }
        say(first);
        return rc;
    }
    // a rank of a SHARDED chain that cannot start a step's proof (its witness failed) takes part in that step's collectives on the failing
    // side: the other ranks' proofs of the step return VPBS_ERR_PEER and the chain ends on every rank instead of hanging on the others
    void abandon_step(int why) {
        if (!cyc.comm) return;
        vpbs_step_inputs shape;
        cyc.step_inputs(shape, nullptr, true, nullptr);
        (void)vpbs_prove_step_sharded_fail(ctx, &shape, cyc.comm, why);
    }
    long stop_step(const std::string& m, int why) {
        abandon_step(why);
        return stop(m, why);
    }
    void lap(double& wall, double& cpu) {   // the section since the last lap
        const double t = now(), c = thread_cpu();
        wall += t - lap_t;
        cpu += c - lap_c;
        lap_t = t;
        lap_c = c;
    }

    // cyclic_base_proof (:292-299): a proof of the dummy circuit carrying the initial accumulator and the cyclic verifier data -- or, on a
    // resume, the checkpoint's proof words.  0, or what stop() returned
    long base(const u64* base_pis) {
        vpbs_step_sizes sz{};
        if (!from && vpbs_witness_plan_run(dum.plan, base_pis, 0, v->base_wires, e, sizeof e) != 0)
            return stop(std::string("dummy witness: ") + e, VPBS_ERR_INVALID);
        dum.step_inputs(in, v->base_wires, false, base_pis);
        if (vpbs_step_sizes_get(ctx, &in, &sz) != 0 || 3 * sz.cap_words + sz.openings_words + sz.fri_words != proof_words)
            return stop("the proof of this shape does not have the number of words the cyclic circuit expects", VPBS_ERR_INVALID);
        openings = caps + 3 * sz.cap_words;
        fri = openings + sz.openings_words;
        if (from) {
            std::memcpy(proof.data(), from_proof, 8 * proof_words);   // the checkpoint's proof is the inner proof of step `from`
        } else {
            const int rc = dum.prove(in, caps, openings, fri);
            if (rc != 0) return stop(std::string("base proof: ") + vpbs_last_error(ctx), rc);
            t_base = now() - t0;
            if (v->step_fn) v->step_fn(v->step_user, 0);
        }
        if (v->staged && !v->dw_late) {
            ahead.ranges = v->ahead_layout.ranges;
            ahead.packed = v->late_vals;
            ahead.start(cyc.plan);
        }
        return 0;
    }
    // on_section of a step's proof with the late phase on the host: the sections of the proof in progress that are final
    static void section(void* user, int sec) {
        auto* r = static_cast<ChainRun*>(user);
        if (r->next.buf < 0) {
            if (!r->src->try_take(r->j + 1, r->next)) return;   // the next step is not staged yet: its late phase runs whole, after the proof
            r->ahead.begin(r->next.state.get(), r->next.values, r->proof.data());
        }
        r->ahead.post((unsigned)sec);
    }
    // local step j: late phase, scatter, proof; then the buffer goes back, the step hook runs and the checkpoint is taken.  0, or what stop() returned
    long step(unsigned local, const StepSource& source) {
        j = local;
        src = &source;
        const unsigned s = from + j;
        cur = std::move(next);
        next = Staged{};
        if (!source.take(j, cur)) return stop_step("", VPBS_ERR_INVALID);
        const std::string late_failed = "late witness phase of step " + std::to_string(s) + " (the previous proof does not verify in circuit): ";
        u64* d_wires = v->d_bufs[cur.buf];
        int rc;
        lap_t = now();
        lap_c = thread_cpu();
        if (v->dw_late) {
            // the late phase on the device object that holds the step's early values, then ALL its wires into the prover's matrix
            const unsigned o = (j / v->dw_batch) & 1, i = j % v->dw_batch;
            rc = vpbs_witness_device_run_late(v->wdev[o], i, proof.data());
            if (rc != 0) return stop_step(late_failed + vpbs_last_error(v->wctx[o]), rc);
            lap(t_late, c_late);
            rc = vpbs_witness_device_wires(v->wdev[o], i, d_wires);
            if (rc != 0) return stop_step(std::string("gathering the wires: ") + vpbs_last_error(v->wctx[o]), rc);
        } else {
            if (ahead.active()) {   // stages that ran ahead on this step's state: wait for the last of them (usually long finished)
                std::string msg;
                if (!ahead.drain(msg)) return stop_step(late_failed + msg, VPBS_ERR_INVALID);
            }
            if (cur.values != proof.data()) std::memcpy(cur.values, proof.data(), 8 * proof_words);   // else the prover wrote them there
            rc = vpbs_witness_plan_run_late_packed(cyc.plan, cur.state.release(), cur.values, v->late_vals, e, sizeof e);   // consumes the state, also when it fails
            if (rc != 0) return stop_step(late_failed + e, rc);
            lap(t_late, c_late);
            // queued, not waited for: the proof is ordered behind it on the context's stream, and the packed buffer is next written a whole
            // proof (several waits on this stream) later -- by the late stages of the NEXT step, which start at this proof's first section
            rc = vpbs::device_scatter(ctx, d_wires, v->d_late_pos, v->late_vals, v->late_count, v->d_late_stage, false);
            if (rc != 0) return stop_step(std::string("upload of the late wires: ") + vpbs_last_error(ctx), rc);
        }
        lap(t_rows, c_rows);
        cyc.step_inputs(in, d_wires, true, cur.pis);
        if (v->staged && s + 1 < steps) {
            static const bool dev_ahead = !std::getenv("VPBS_DEVICE_LATE_AHEAD") || std::atoi(std::getenv("VPBS_DEVICE_LATE_AHEAD")) != 0;   // A-B switch
            if (!v->dw_late) {
                in.on_section = &ChainRun::section;
                in.on_section_user = this;
            } else if (dev_ahead) {
                source.arm_device_late(j, in);
            }
        }
        rc = cyc.prove(in, caps, openings, fri);
        if (rc != 0) {   // a sharded chain's collectives carried it already
            if (ahead.active()) {   // the worker may be inside a stage of the next step's state: let it finish before that state is freed
                std::string ignored;
                (void)ahead.drain(ignored);
            }
            return stop("step " + std::to_string(s) + ": " + vpbs_last_error(ctx), rc);
        }
        lap(t_prove, c_prove);
        source.release(j, cur);
        if (v->step_fn) v->step_fn(v->step_user, s + 1);
        if (v->checkpoint(in, caps, openings, fri, s + 1, steps) != 0) return stop("checkpoint after step " + std::to_string(s) + ": the proof does not serialise", VPBS_ERR_INVALID);
        return 0;
    }
    // the last proof serialised (ProofWithPublicInputs::to_bytes) and the timing of the run
    long tail(const StepSource& source) {
        join();
        const double seconds = now() - t0;
        if (source.waits && std::getenv("VPBS_TRACE_IVC"))
            std::fprintf(stderr, "[ivc device witness] per step: waited %.2f ms for the staged wires, %.2f ms for the hash chain; late %.2f, scatter %.2f, "
                         "prove %.2f, device batch run %.2f ms; CPU time of the proving thread: late %.2f, scatter %.2f, prove %.2f ms (blocking waits: %d)\n",
                         1e3 * source.waits[0] / n_run, 1e3 * source.waits[1] / n_run, 1e3 * t_late / n_run, 1e3 * t_rows / n_run, 1e3 * t_prove / n_run,
                         1e3 * t_early / n_run, 1e3 * c_late / n_run, 1e3 * c_rows / n_run, 1e3 * c_prove / n_run, vpbs_host_blocking_sync());
        const long n_bytes = v->to_bytes(in, caps, openings, fri, proof_out, capacity);
        if (n_bytes <= 0) {
            say("the output buffer is too small for the proof");
            return VPBS_ERR_INVALID;
        }
        if (timing) {
            timing->seconds = seconds;
            timing->steps = n_run;
            timing->base_proof_ms = 1e3 * t_base;
            timing->late_witness_ms = 1e3 * t_late / n_run;
            timing->late_rows_upload_ms = 1e3 * t_rows / n_run;
            timing->prove_step_ms = 1e3 * t_prove / n_run;
            timing->early_witness_ms = 1e3 * t_early / n_run;
            timing->late_ahead_ms = 1e3 * ahead.busy_s / n_run;
        }
        return n_bytes;
    }
    long run(const u64* base_pis, const StepSource& source) {
        long rc = base(base_pis);
        for (unsigned k = 0; rc == 0 && k < n_run; ++k) rc = step(k, source);
        return rc == 0 ? tail(source) : rc;
    }
};
}  // namespace

extern "C" {

int vpbs_ivc_create(vpbs_ctx* ctx, const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, unsigned N, unsigned K, size_t ggsw_len,
                    const vpbs_comm* comm, vpbs_ivc** out, char* err, size_t err_len) {
    auto say = [&](const std::string& m) { report(err, err_len, m); };
    say("");
    if (!ctx || !cyclic || !dummy || !out || !cyclic->circuit || !dummy->circuit || !cyclic->preset_pos || !dummy->preset_pos || !cyclic->pi_pos ||
        N == 0 || K == 0) {
        say("malformed arguments");
        return VPBS_ERR_INVALID;
    }
    // the proofs of the chain are proofs under CircuitConfig::standard_recursion_config (ivc_based_vpbs.rs:190): rate 1/8, cap height 4 -- the
    // in-circuit verifier of the cyclic circuit is built for that shape (16 cap entries in the verifier data and in every proof), so a
    // context of another shape cannot prove it: its commitments would carry another cap and every vk derived here would be wrong
    const unsigned cap_height = vpbs_ctx_cap_height(ctx);
    if (vpbs_ctx_rate_bits(ctx) != 3 || cap_height != 4) {
        say("the IVC chain needs a context with rate_bits = 3 and cap_height = 4 (standard_recursion_config)");
        return VPBS_ERR_INVALID;
    }
    const size_t kn = (size_t)K * N, cap_words = (size_t)4 << cap_height, n_pi = 2 * kn + 9 + 4 + cap_words;
    // the PartialWitness of a step, in the order the reference sets it (:314-330): previous proof | its public inputs | condition | GGSW |
    // mask | own verifier data | then what plonky2's DummyProofGenerator sets: dummy verifier data | the dummy circuit's proof | its public
    // inputs (the second proof slot of conditionally_verify_cyclic_proof_or_dummy); the dummy circuit's PartialWitness is its public inputs
    if (cyclic->n_pi != n_pi || dummy->n_preset != n_pi || (dummy->n_pi != 0 && dummy->n_pi != n_pi) ||
        cyclic->n_preset != 2 * (cyclic->proof_words + n_pi) + 1 + ggsw_len + 1 + 2 * (4 + cap_words)) {
        say("the circuits are not a cyclic step circuit and its dummy circuit for these parameters (public inputs / PartialWitness layout)");
        return VPBS_ERR_INVALID;
    }
    auto* v = new vpbs_ivc();
    v->ctx = ctx; v->N = N; v->K = K; v->ggsw_len = ggsw_len; v->kn = kn; v->n_pi = n_pi; v->proof_words = cyclic->proof_words;
    if (comm) v->comm = *comm;   // the callbacks and staging buffers stay the caller's; the struct itself is copied
    int rc = v->cyc.init(ctx, *cyclic, cap_height, comm ? &v->comm : nullptr, v->err);
    if (rc == 0) rc = v->dum.init(ctx, *dummy, cap_height, nullptr, v->err);   // the base proof is small: every rank proves it whole
    v->dum.n_pi = n_pi;   // the base proof carries the cyclic circuit's public-input layout whatever the caller wrote into dummy->n_pi
    if (rc == 0) {
        std::vector<uint8_t> late(cyclic->n_preset, 0);
        std::fill(late.begin(), late.begin() + cyclic->proof_words, 1);
        // the proof's sections as late STAGES (LateAhead); VPBS_IVC_LATE_STAGES=0: one late phase after the proof, as in rounds 2-3 (A-B runs)
        const char* ev = std::getenv("VPBS_IVC_LATE_STAGES");
        if (!(ev && std::atoi(ev) == 0)) {
            vpbs_fri_params fp;
            vpbs_fri_params_standard(v->cyc.log_n, &fp);
            unsigned final_bits = v->cyc.log_n;
            for (unsigned i = 0; i < fp.n_rounds; ++i) final_bits -= fp.arity_bits[i];
            vpbs_step_inputs shape;
            vpbs_step_sizes sz{};
            v->cyc.step_inputs(shape, nullptr, true, nullptr);
            const size_t fri_fixed = (size_t)fp.n_rounds * cap_words + ((size_t)2 << final_bits) + 1;
            if (vpbs_step_sizes_get(ctx, &shape, &sz) == 0 && sz.cap_words == cap_words &&
                3 * sz.cap_words + sz.openings_words + sz.fri_words == cyclic->proof_words && sz.fri_words > fri_fixed) {
                v->ahead_layout.layout(cap_words, sz.openings_words, sz.fri_words, fp.n_rounds, (size_t)2 << final_bits, late);
                v->staged = true;
            }
        }
        char e[256] = {0};
        rc = vpbs_witness_plan_split(v->cyc.plan, late.data(), e, sizeof e);
        if (rc != 0) v->err = std::string("split: ") + e;
        if (rc == 0) rc = vpbs_witness_plan_late_rows(v->cyc.plan, v->late_rows);
        if (rc == 0) v->late_count = vpbs_witness_plan_late_count(v->cyc.plan);
    }
    if (rc == 0) {
        v->wire_words = (size_t)v->cyc.n_wires * v->cyc.n;
        for (auto& b : v->bufs)
            if (!(b = static_cast<u64*>(vpbs_host_alloc(8 * v->wire_words)))) rc = VPBS_ERR_OOM;
        for (auto& d : v->d_bufs)
            if (rc == 0) rc = vpbs_device_alloc(ctx, v->wire_words, &d);
        if (!(v->base_wires = static_cast<u64*>(vpbs_host_alloc(8 * (size_t)v->dum.n_wires * v->dum.n)))) rc = VPBS_ERR_OOM;
        // the late phase's values travel packed (a few MB per step instead of the row range of all 135 columns) and are scattered on the device
        if (rc == 0 && v->late_count) {
            const size_t pos_words = (v->late_count + 1) / 2;
            if (!(v->late_vals = static_cast<u64*>(vpbs_host_alloc(8 * std::max(v->late_count, pos_words))))) rc = VPBS_ERR_OOM;
            if (rc == 0) rc = vpbs_device_alloc(ctx, pos_words, &v->d_late_pos);
            if (rc == 0) rc = vpbs_device_alloc(ctx, v->late_count, &v->d_late_stage);
            if (rc == 0) rc = vpbs_witness_plan_late_positions(v->cyc.plan, reinterpret_cast<uint32_t*>(v->late_vals));
            if (rc == 0) rc = vpbs_device_upload(ctx, v->d_late_pos, v->late_vals, pos_words);
        }
        if (rc != 0) v->err = "wire matrices: out of (pinned or device) memory";
    }
    if (rc == 0) {
        // dummy_proof_and_vk (recursion/dummy_circuit.rs): the dummy circuit's proof of all-zero public inputs -- the content of the second
        // proof slot in every step of every chain, so it is proven once here
        char e[256] = {0};
        const std::vector<u64> zero_pis(n_pi, 0);
        vpbs_step_inputs in;
        vpbs_step_sizes sz{};
        if (vpbs_witness_plan_run(v->dum.plan, zero_pis.data(), 0, v->base_wires, e, sizeof e) != 0) {
            v->err = std::string("dummy witness: ") + e;
            rc = VPBS_ERR_INVALID;
        }
        if (rc == 0) {
            v->dum.step_inputs(in, v->base_wires, false, zero_pis.data());
            if (vpbs_step_sizes_get(ctx, &in, &sz) != 0 || 3 * sz.cap_words + sz.openings_words + sz.fri_words != v->proof_words) {
                v->err = "the proof of this shape does not have the number of words the cyclic circuit expects";
                rc = VPBS_ERR_INVALID;
            }
        }
        if (rc == 0) {
            v->dummy_proof.assign(v->proof_words, 0);
            u64 *caps = v->dummy_proof.data(), *openings = caps + 3 * sz.cap_words, *fri = openings + sz.openings_words;
            rc = v->dum.prove(in, caps, openings, fri);
            if (rc != 0) v->err = std::string("dummy proof: ") + vpbs_last_error(ctx);
        }
    }
    if (rc != 0) {
        say(v->err);
        delete v;
        return rc;
    }
    *out = v;
    return VPBS_OK;
}

void vpbs_ivc_free(vpbs_ivc* v) { delete v; }

int vpbs_ivc_set_step_callback(vpbs_ivc* v, vpbs_ivc_step_fn fn, void* user) {
    if (!v) return VPBS_ERR_INVALID;
    v->step_fn = fn;
    v->step_user = user;
    return VPBS_OK;
}

const char* vpbs_ivc_last_error(const vpbs_ivc* v) { return v ? v->err.c_str() : ""; }

int vpbs_ivc_set_check_witness(vpbs_ivc* v, int on) {
    if (!v) return VPBS_ERR_INVALID;
    v->err.clear();
    if (on && v->cyc.comm) {   // a rank that stopped after its collectives began would leave its peers waiting
        v->err = "witness checking is not available for a sharded chain";
        return VPBS_ERR_INVALID;
    }
    v->checks[0] = v->checks[1] = 0;
    int rc = v->cyc.set_check(on != 0, v->checks, v->err);
    if (rc == VPBS_OK) rc = v->dum.set_check(on != 0, v->checks, v->err);
    if (rc != VPBS_OK) {
        std::string keep;
        (void)v->cyc.set_check(false, v->checks, keep);
        (void)v->dum.set_check(false, v->checks, keep);
    }
    return rc;
}

int vpbs_ivc_witness_checks(const vpbs_ivc* v, uint64_t out[2]) {
    if (!v || !out) return VPBS_ERR_INVALID;
    out[0] = v->checks[0];
    out[1] = v->checks[1];
    return VPBS_OK;
}

int vpbs_ivc_verifier_data(const vpbs_ivc* v, uint64_t* cyclic_vk, uint64_t* dummy_vk) {
    if (!v) return VPBS_ERR_INVALID;
    if (cyclic_vk) std::memcpy(cyclic_vk, v->cyc.vk.data(), 8 * v->cyc.vk.size());
    if (dummy_vk) std::memcpy(dummy_vk, v->dum.vk.data(), 8 * v->dum.vk.size());
    return VPBS_OK;
}

int vpbs_ivc_set_device_witness(vpbs_ivc* v, unsigned ELL, unsigned LOGB, unsigned batch, int late_on_device) {
    if (!v) return VPBS_ERR_INVALID;
    v->drop_device_witness();
    v->dw_late = false;
    v->err.clear();
    if (batch == 0) return VPBS_OK;
    if (ELL == 0 || LOGB == 0 || v->ggsw_len != (size_t)v->K * ELL * v->K * v->N) {
        v->err = "device witness: ELL / LOGB do not fit the circuit's GGSW length";
        return VPBS_ERR_INVALID;
    }
    int rc = VPBS_OK;
    for (int i = 0; i < 2 && rc == 0; ++i) {
        rc = vpbs_ctx_create(vpbs_ctx_device(v->ctx), v->cyc.log_n, vpbs_ctx_rate_bits(v->ctx), vpbs_ctx_cap_height(v->ctx), &v->wctx[i]);
        if (rc == 0) rc = vpbs_witness_device_create_early(v->wctx[i], v->cyc.plan, batch, &v->wdev[i]);
        if (rc != 0) v->err = std::string("device witness: ") + (v->wctx[i] ? vpbs_last_error(v->wctx[i]) : "no context");
        if (rc == 0 && late_on_device && !vpbs_witness_device_has_late(v->wdev[i])) {
            v->err = "device witness: late_on_device was requested, but the late phase of this circuit has no device schedule (a late generator "
                     "without a device form); use late_on_device = 0";
            rc = VPBS_ERR_INVALID;
        }
    }
    if (rc == 0 && !(v->dw_presets = static_cast<u64*>(vpbs_host_alloc(8 * v->cyc.n_preset * (size_t)batch)))) {
        v->err = "device witness: out of pinned memory";
        rc = VPBS_ERR_OOM;
    }
    if (rc != 0) {
        v->drop_device_witness();
        return rc;
    }
    v->late_in_count = vpbs_witness_plan_late_input_count(v->cyc.plan);
    v->ELL = ELL; v->LOGB = LOGB; v->dw_batch = batch;
    v->dw_late = late_on_device != 0;
    return VPBS_OK;
}

// The early-phase preset matrix [n_preset][cnt] (instances innermost: what vpbs_witness_device_run takes) of chain steps
// [first, first + cnt): previous proof (late: ignored by the early phase, zeros) | the predecessor's public inputs | condition | GGSW | mask |
// own and dummy verifier data | the dummy proof | its public inputs (zeros).  pis: [cnt][n_pi], the public inputs of the predecessors of
// those steps.  The host statement of the layout (tests reach it through vpbs_test_ivc_preset_matrix); csrc/pbs_prove_batch.hip assembles the same
// matrix on the device.
static void preset_matrix_host(u64* m, unsigned first, unsigned cnt, const u64* pis, size_t proof_words, size_t n_pi, size_t ggsw_len, unsigned n_lwe,
                               const u64* ct, const u64* bsk, const u64* ksk, const u64* cyc_vk, const u64* dum_vk, size_t vk_words,
                               const u64* dummy_proof) {
    auto row = [&](size_t r) { return m + r * cnt; };
    for (size_t r = 0; r < proof_words; ++r) std::memset(row(r), 0, 8 * cnt);
    for (unsigned i = 0; i < cnt; ++i) {
        const unsigned s = first + i;
        const u64* q = pis + (size_t)i * n_pi;
        size_t r = proof_words;
        for (size_t k = 0; k < n_pi; ++k) row(r++)[i] = q[k];
        row(r++)[i] = s == 0 ? 0 : 1;
        const u64* g = s == 0 ? nullptr : (s <= n_lwe ? bsk + (size_t)(s - 1) * ggsw_len : ksk);
        for (size_t k = 0; k < ggsw_len; ++k) row(r++)[i] = g ? g[k] : 0;
        row(r++)[i] = s == 0 ? ct[n_lwe] : (s <= n_lwe ? ct[s - 1] : (u64)0);
        for (size_t k = 0; k < vk_words; ++k) row(r++)[i] = cyc_vk[k];
        for (size_t k = 0; k < vk_words; ++k) row(r++)[i] = dum_vk[k];
        for (size_t k = 0; k < proof_words; ++k) row(r++)[i] = dummy_proof[k];
        for (size_t k = 0; k < n_pi; ++k) row(r++)[i] = 0;
    }
}

// The chain with the early witness phases on the device.  What a step's early phase needs of its predecessor are the predecessor's PUBLIC
// INPUTS, and those are known without proving anything: the accumulators from the native chain (vpbs_pbs_accumulator_chain), the two chain
// hashes from the native sponge (one host thread walks them ahead of the batches), counter and verifier data.  So the early phases of
// `dw_batch` consecutive steps run on the device at once (thread B), a stager thread gathers an instance's wires into the device matrix
// the prover will read and fetches the early values the late phase needs (thread S), and the loop (ChainRun, which this function only
// feeds with staged steps) is left with the late phase (the in-circuit verifier's rows), the scatter of its values and the proof.
// from > 0 (vpbs_ivc_resume_pbs): no base proof; step `from` takes the checkpoint's proof words and public inputs, the native accumulator
// chain starts at step `from` from the checkpoint's accumulator and the hash thread from its two hashes.  Progress below is counted in steps
// of THIS call: local step j is chain step from + j.
// res != nullptr (vpbs::ivc_prove_pbs_resident, bsk and ksk not read): the chain's public inputs exist already -- accumulators and both hash
// chains are taken from `res`, indexed by ABSOLUTE chain step whatever `from` is, and every batch's preset matrix is written on the device by
// res->fill, called with the absolute first step.
static long prove_pbs_device_witness(const ChainArgs& a, const vpbs::IvcResidentChain* res = nullptr) {
    ChainRun run(a);   // the clock starts here
    vpbs_ivc* v = a.v;
    Side &cyc = v->cyc, &dum = v->dum;
    const size_t kn = v->kn, n_pi = v->n_pi, ggsw_len = v->ggsw_len;
    const unsigned B = v->dw_batch, from = a.from, n_lwe = a.n_lwe, total = n_lwe + 2, n_run = run.n_run;
    constexpr unsigned NBUF = vpbs_ivc::NBUF;
    std::mutex& mu = run.mu;
    std::condition_variable& cv = run.cv;
    std::atomic<bool>& failed = run.failed;
    auto fail = [&](const std::string& m) { run.fail(m); };
    // ---- the chain's public inputs, natively ----
    // accs[j] = the accumulator after chain step from + j (step `from` reads acc_init, or the checkpoint's accumulator)
    std::vector<u64> acc_init(kn, 0), own_accs(res ? 0 : (size_t)(total - from) * kn);
    std::memcpy(acc_init.data() + kn - v->N, a.testv, 8 * (size_t)v->N);
    unsigned log_N = 0;
    while ((1u << log_N) < v->N) ++log_N;
    const vpbs_tfhe_params tp{log_N, v->K, v->ELL, v->LOGB};
    if (!res && vpbs::pbs_accumulator_chain_from(v->ctx, &tp, n_lwe, from, from ? a.from_pis + kn + 1 : acc_init.data(), a.ct, a.bsk, a.ksk, own_accs.data()) != 0) {
        run.say(std::string("native accumulator chain: ") + vpbs_last_error(v->ctx));
        return VPBS_ERR_INVALID;
    }
    const u64* accs = res ? res->accs + (size_t)from * kn : own_accs.data();   // accs[j]: after chain step from + j (valid from j = -1 for res)
    // pis[j + 1] = public inputs of step from + j (pis[0]: of the base proof, or the checkpoint's): acc_init | counter | accumulator | key
    // hash | LWE hash | verifier data
    std::vector<u64> pis((size_t)(n_run + 1) * n_pi, 0);
    for (unsigned j = 0; j <= n_run; ++j) {
        u64* q = pis.data() + (size_t)j * n_pi;
        if (j == 0 && from) {
            std::memcpy(q, a.from_pis, 8 * n_pi);
            continue;
        }
        std::memcpy(q, acc_init.data(), 8 * kn);
        q[kn] = from + j;
        if (j) std::memcpy(q + kn + 1, accs + ((size_t)j - 1) * kn, 8 * kn);
        std::memcpy(q + n_pi - cyc.vk.size(), cyc.vk.data(), 8 * cyc.vk.size());
    }
    unsigned hashed = 0;        // steps whose chain hashes are in pis (guarded by mu; these four count the steps of this call: local j)
    unsigned batches_run = 0;   // batches whose early phases are on the device
    unsigned staged = 0;        // steps gathered and read back
    unsigned consumed = 0;      // steps the loop has finished with (their device matrix is free again)
    // thread H: the two hash chains of verify_hash_output (:64-78), h_s = hash_no_pad(h_{s-1} || item_s), one permutation after the other
    run.spawn("vpbs-hash", [&] {
        if (res) {   // both chains exist: nothing to wait for, nothing to hash
            for (unsigned s = 0; s < n_run; ++s) {
                u64* q = pis.data() + (size_t)(s + 1) * n_pi + 2 * kn + 1;
                std::memcpy(q, res->key_links + 4 * (size_t)(from + s), 32);
                std::memcpy(q + 4, res->lwe_links + 4 * (size_t)(from + s), 32);
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                hashed = n_run;
            }
            cv.notify_all();
            return;
        }
        std::vector<u64> in2(5);
        u64 hb[4], hl[4];   // the chains so far: zero before the base proof, the checkpoint's hashes on a resume
        std::memcpy(hb, pis.data() + 2 * kn + 1, 32);
        std::memcpy(hl, pis.data() + 2 * kn + 5, 32);
        // the key chain in segments of eight links: the chains of one process walk theirs side by side (vpbs_hash_chain_links)
        constexpr unsigned SEG = 8;
        const u64* items[SEG];
        u64 links[4 * SEG];
        for (unsigned s0 = 0; s0 < n_run && !failed; s0 += SEG) {
            {   // three batches ahead of the chain, no further: the batcher needs two, and the chains' hashing is spread over their whole
                // length instead of a burst of 1.9 s of CPU per chain at the start (which a timed window further on would not see)
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed || s0 < consumed + 3 * B; });
                if (failed) return;
            }
            const unsigned cnt = std::min(SEG, n_run - s0);
            for (unsigned i = 0; i < cnt; ++i) items[i] = run.ggsw_of(from + s0 + i);
            if (vpbs_hash_chain_links(hb, items, cnt, ggsw_len, links) != 0) return fail("hash chain of the bootstrapping key: malformed arguments");
            std::memcpy(hb, links + 4 * (cnt - 1), 32);
            for (unsigned i = 0; i < cnt; ++i) {
                const unsigned s = s0 + i;
                std::memcpy(in2.data(), hl, 32);
                in2[4] = run.mask_of(from + s);
                vpbs_hash_no_pad(in2.data(), 5, hl);
                u64* q = pis.data() + (size_t)(s + 1) * n_pi + 2 * kn + 1;
                std::memcpy(q, links + 4 * i, 32);
                std::memcpy(q + 4, hl, 32);
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                hashed = s0 + cnt;
            }
            cv.notify_all();
        }
    });
    // thread B: batch b = steps [b B, (b + 1) B) on device object b & 1, once their public inputs exist and the object's previous batch is consumed
    const unsigned n_batches = (n_run + B - 1) / B;
    run.spawn("vpbs-batcher", [&] {
        for (unsigned b = 0; b < n_batches && !failed; ++b) {
            const unsigned first = b * B, cnt = std::min(B, n_run - first);
            {
                std::unique_lock<std::mutex> lk(mu);
                // step s needs the public inputs of step s - 1: hashed >= first + cnt - 1; the object held batch b - 2
                cv.wait(lk, [&] { return failed || (hashed + 1 >= first + cnt && (b < 2 || consumed >= (b - 1) * B)); });
                if (failed) return;
            }
            const double t = now();
            int run_rc;
            if (res) {   // the matrix is assembled on the device, on the witness object's stream
                struct Fill {
                    const vpbs::IvcResidentChain* res;
                    unsigned first, cnt;
                    static int call(void* user, void* stream, uint64_t* d_matrix) {
                        auto* f = static_cast<Fill*>(user);
                        return f->res->fill(f->res->user, stream, f->first, f->cnt, d_matrix);
                    }
                } fill{res, from + first, cnt};
                run_rc = vpbs::witness_device_run_filled(v->wdev[b & 1], cnt, &Fill::call, &fill);
            } else {
                u64* m = v->dw_presets;   // [n_preset][cnt]
                preset_matrix_host(m, from + first, cnt, pis.data() + (size_t)first * n_pi, v->proof_words, n_pi, ggsw_len, n_lwe, a.ct, a.bsk, a.ksk,
                                   cyc.vk.data(), dum.vk.data(), cyc.vk.size(), v->dummy_proof.data());
                run_rc = vpbs_witness_device_run(v->wdev[b & 1], m, cnt);
            }
            if (run_rc != 0)
                return fail("early witness phases of steps " + std::to_string(from + first) + ".. on the device: " + vpbs_last_error(v->wctx[b & 1]));
            run.t_early += now() - t;
            {
                std::lock_guard<std::mutex> lk(mu);
                batches_run = b + 1;
            }
            cv.notify_all();
        }
    });
    // thread S: per step, the instance's wires into one of the device matrices, the late phase's inputs to the host and the late phase's
    // state seeded with them (allocation and first touch of its pages happen here, ahead of the chain)
    std::vector<std::vector<u64>> late_in(NBUF, std::vector<u64>(v->late_in_count));
    State states[NBUF];   // owned here until the loop takes one; whatever is left at the end is freed
    run.spawn("vpbs-stager", [&] {
        if (v->dw_late) return;   // the loop runs the late phase on the device object itself and gathers afterwards
        for (unsigned j = 0; j < n_run && !failed; ++j) {
            const unsigned b = j / B, k = j % NBUF;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed || (batches_run > b && j < consumed + NBUF); });
                if (failed) return;
            }
            if (vpbs_witness_device_wires(v->wdev[b & 1], j % B, v->d_bufs[k]) != 0 ||
                vpbs_witness_device_read_late_inputs(v->wdev[b & 1], j % B, late_in[k].data()) != 0)
                return fail("gathering the early wires of step " + std::to_string(from + j) + ": " + vpbs_last_error(v->wctx[b & 1]));
            vpbs_witness_state* st = nullptr;
            if (vpbs_witness_state_from_late_inputs(cyc.plan, late_in[k].data(), &st) != 0)
                return fail("late witness phase of step " + std::to_string(from + j) + ": the early values read back from the device are malformed");
            {
                std::lock_guard<std::mutex> lk(mu);
                states[k].reset(st);
                staged = j + 1;
            }
            cv.notify_all();
        }
    });
    // The LateAhead idea with the late phase on the DEVICE (round 6): the stages of the next step's late phase are queued on its witness object's
    // stream as the sections of the proof in progress become final (the prover writes them straight into the loop's proof buffer); when the
    // proof returns only the last stage -- the query rounds: 33 of the 162 dependency levels -- is left to queue and wait for.
    struct DevHook {
        vpbs_ivc* v;
        std::mutex* mu;
        const unsigned* batches_run;
        unsigned B;
        const u64* values;
        unsigned step = 0, queued = 0;   // the step being proven; stages of step + 1 queued so far
        static void section(void* user, int sec) {
            auto* h = static_cast<DevHook*>(user);
            const unsigned next = h->step + 1;
            {
                std::lock_guard<std::mutex> lk(*h->mu);
                if (*h->batches_run <= next / h->B) return;   // the next step's early batch has not run yet: its late phase runs whole, after the proof
            }
            vpbs_witness_device* dev = h->v->wdev[(next / h->B) & 1];
            const unsigned n = vpbs::witness_device_late_stages(dev);
            while (h->queued < (unsigned)sec && h->queued + 1 < n) {   // the last stage waits for the return
                if (vpbs::witness_device_run_late_stage(dev, next % h->B, h->queued + 1, h->values, 0) != 0) return;   // run_late reports it
                ++h->queued;
            }
        }
    } dev_hook{v, &mu, &batches_run, B, run.proof.data()};
    double waits[2] = {0, 0};
    auto hand_over = [&](unsigned j, Staged& step) {   // mu held, step j staged
        step.buf = j % NBUF;
        step.pis = pis.data() + (size_t)(j + 1) * n_pi;
        step.values = run.proof.data();
        step.state = std::move(states[j % NBUF]);   // none with the late phase on the device
    };
    StepSource src;
    src.waits = waits;
    src.take = [&](unsigned j, Staged& step) {
        const double tw = now();
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || (v->dw_late ? batches_run > j / B : staged > j); });
        const double tw2 = now();
        waits[0] += tw2 - tw;
        cv.wait(lk, [&] { return failed || hashed > j; });   // its own public inputs are complete
        waits[1] += now() - tw2;
        if (failed) return false;
        if (step.buf < 0) hand_over(j, step);
        return true;
    };
    src.try_take = [&](unsigned j, Staged& step) {
        std::lock_guard<std::mutex> lk(mu);
        if (staged <= j) return false;
        hand_over(j, step);
        return true;
    };
    src.release = [&](unsigned j, const Staged&) {
        {
            std::lock_guard<std::mutex> lk(mu);
            consumed = j + 1;
        }
        cv.notify_all();
    };
    src.arm_device_late = [&](unsigned j, vpbs_step_inputs& in) {
        dev_hook.step = j;
        dev_hook.queued = 0;
        in.on_section = &DevHook::section;
        in.on_section_user = &dev_hook;
    };
    return run.run(pis.data(), src);
}

// The host pipeline (the default): early phase on thread E, upload on thread U, late phase + proof in the loop (ChainRun).  from > 0
// (vpbs_ivc_resume_pbs): no base proof; step `from` takes the checkpoint's proof words and public inputs.
static long prove_pbs_host(const ChainArgs& a) {
    ChainRun run(a);
    vpbs_ivc* v = a.v;
    Side &cyc = v->cyc, &dum = v->dum;
    const size_t kn = v->kn, n_pi = v->n_pi;
    std::mutex& mu = run.mu;
    std::condition_variable& cv = run.cv;
    std::atomic<bool>& failed = run.failed;
    // public inputs of the base proof: acc_init = (0, .., 0, testv) | counter 0 | accumulator 0 | hashes 0 | the cyclic circuit's verifier data
    std::vector<u64> base_pis(n_pi, 0);
    std::memcpy(base_pis.data() + kn - v->N, a.testv, 8 * (size_t)v->N);
    std::memcpy(base_pis.data() + n_pi - cyc.vk.size(), cyc.vk.data(), 8 * cyc.vk.size());
    std::deque<int> free_bufs{0, 1, 2};
    std::deque<Staged> generated, ready;   // early thread -> uploader -> the loop; whatever nobody consumed is freed at the end
    run.spawn("vpbs-early", [&] {
        std::vector<u64> pis_prev = a.from ? std::vector<u64>(a.from_pis, a.from_pis + n_pi) : base_pis;
        char e2[256];
        for (unsigned s = a.from; s < a.steps && !failed; ++s) {
            Staged r;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !free_bufs.empty() || failed; });
                if (failed) return;
                r.buf = free_bufs.front();
                free_bufs.pop_front();
            }
            const double t = now();
            std::vector<u64>& vals = r.own_values;
            vals.reserve(cyc.n_preset);
            vals.assign(v->proof_words, 0);
            vals.insert(vals.end(), pis_prev.begin(), pis_prev.end());
            vals.push_back(s == 0 ? 0 : 1);   // condition: false only in the base step
            vals.insert(vals.end(), run.ggsw_of(s), run.ggsw_of(s) + v->ggsw_len);
            vals.push_back(run.mask_of(s));
            vals.insert(vals.end(), cyc.vk.begin(), cyc.vk.end());
            vals.insert(vals.end(), dum.vk.begin(), dum.vk.end());
            vals.insert(vals.end(), v->dummy_proof.begin(), v->dummy_proof.end());
            vals.insert(vals.end(), n_pi, 0);   // the dummy proof's public inputs
            r.values = vals.data();
            // a matrix this plan has filled before only gets its value-carrying positions rewritten
            const auto run_early = v->filled[r.buf] ? vpbs_witness_plan_run_early_recycled : vpbs_witness_plan_run_early;
            vpbs_witness_state* st = nullptr;
            const int rc = run_early(cyc.plan, r.values, 0, v->bufs[r.buf], &st, e2, sizeof e2);
            r.state.reset(st);
            if (rc != 0) return run.fail("early witness phase of step " + std::to_string(s) + ": " + e2);
            v->filled[r.buf] = true;
            r.own_pis.resize(n_pi);
            for (size_t i = 0; i < n_pi; ++i) r.own_pis[i] = v->bufs[r.buf][cyc.pi_pos[i]];   // public inputs never depend on the inner proof's words
            r.pis = r.own_pis.data();
            pis_prev = r.own_pis;
            run.t_early += now() - t;
            {
                std::lock_guard<std::mutex> lk(mu);
                generated.push_back(std::move(r));
            }
            cv.notify_all();
        }
    });
    run.spawn("vpbs-upload", [&] {
        for (unsigned s = a.from; s < a.steps; ++s) {
            Staged r;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !generated.empty() || failed; });
                if (failed) return;
                r = std::move(generated.front());
                generated.pop_front();
            }
            if (vpbs_device_upload_bg(v->ctx, v->d_bufs[r.buf], v->bufs[r.buf], v->wire_words) != 0)
                return run.fail("upload of the early wires of step " + std::to_string(s));
            {
                std::lock_guard<std::mutex> lk(mu);
                ready.push_back(std::move(r));
            }
            cv.notify_all();
        }
    });
    auto take_ready = [&](Staged& step) {   // mu held, ready not empty
        step = std::move(ready.front());
        ready.pop_front();
    };
    StepSource src;
    src.take = [&](unsigned, Staged& step) {
        if (step.buf >= 0) return true;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready.empty() || failed; });
        if (failed) return false;
        take_ready(step);
        return true;
    };
    src.try_take = [&](unsigned, Staged& step) {
        std::lock_guard<std::mutex> lk(mu);
        if (ready.empty()) return false;   // its early phase is still running
        take_ready(step);
        return true;
    };
    src.release = [&](unsigned, const Staged& step) {
        {
            std::lock_guard<std::mutex> lk(mu);
            free_bufs.push_back(step.buf);
        }
        cv.notify_all();
    };
    run.t0 = now();
    return run.run(base_pis.data(), src);
}

long vpbs_ivc_prove_pbs(vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, const uint64_t* bsk, const uint64_t* ksk, unsigned n_lwe,
                        unsigned steps, uint8_t* proof_out, size_t capacity, vpbs_ivc_timing* timing, char* err, size_t err_len) {
    report(err, err_len, "");
    if (!v || !testv || !ct || !ksk || (n_lwe && !bsk) || !proof_out) {
        report(err, err_len, "malformed arguments");
        return VPBS_ERR_INVALID;
    }
    const ChainArgs a{v, testv, ct, bsk, ksk, n_lwe, 0, nullptr, nullptr, clamp_steps(steps, n_lwe), proof_out, capacity, timing, err, err_len};
    return v->dw_batch ? prove_pbs_device_witness(a) : prove_pbs_host(a);
}

int vpbs_test_ivc_preset_matrix(size_t proof_words, size_t n_pi, size_t ggsw_len, size_t vk_words, unsigned n_lwe, unsigned first, unsigned count,
                                const uint64_t* pis, const uint64_t* ct, const uint64_t* bsk, const uint64_t* ksk, const uint64_t* cyclic_vk,
                                const uint64_t* dummy_vk, const uint64_t* dummy_proof, uint64_t* out) {
    if (!pis || !ct || !ksk || (n_lwe && !bsk) || !cyclic_vk || !dummy_vk || !dummy_proof || !out || count == 0 || first + count > n_lwe + 2 ||
        first + count < first)
        return VPBS_ERR_INVALID;
    preset_matrix_host(out, first, count, pis, proof_words, n_pi, ggsw_len, n_lwe, ct, bsk, ksk, cyclic_vk, dummy_vk, vk_words, dummy_proof);
    return VPBS_OK;
}

int vpbs_ivc_set_checkpoint(vpbs_ivc* v, unsigned every, vpbs_ivc_checkpoint_fn fn, void* user) {
    if (!v) return VPBS_ERR_INVALID;
    v->ckpt_every = fn ? every : 0;
    v->ckpt_fn = every ? fn : nullptr;
    v->ckpt_user = user;
    return VPBS_OK;
}

// Resume: the checkpoint is the last proof of a prefix of k steps, and its public inputs are the whole state step k reads.  The prefix form
// of verify_pbs against this object's own verifier data establishes that state (by the proof's soundness its accumulator is the right one
// once its hash chains are those of these keys and this ciphertext), so the chain goes on at step k with the checkpoint's proof words as
// step k's inner proof -- the same witnesses, hence the same proofs, as an uninterrupted chain.  The key chain (seconds) runs on a thread of
// its own beside the first resumed steps; everything else is checked before anything is queued.
long vpbs_ivc_resume_pbs(vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, const uint64_t* bsk, const uint64_t* ksk, unsigned n_lwe,
                         const uint8_t* checkpoint, size_t len, unsigned steps, uint8_t* proof_out, size_t capacity, vpbs_ivc_timing* timing,
                         char* err, size_t err_len) {
    auto say = [&](const std::string& m) { report(err, err_len, m); };
    say("");
    if (!v || !testv || !ct || !ksk || (n_lwe && !bsk) || !proof_out || !checkpoint) {
        say("malformed arguments");
        return VPBS_ERR_INVALID;
    }
    if (v->cyc.comm) {
        say("resume is not available for a sharded chain");
        return VPBS_ERR_INVALID;
    }
    const size_t kn = v->kn;
    const vpbs_verify_pbs_inputs pin{nullptr, v->N, v->K, n_lwe, v->ggsw_len, testv, nullptr, ct, bsk, ksk};   // for the key chain alone
    const double t0 = now();
    vpbs::IvcCheckpoint cp;
    std::string why;
    if (!vpbs::ivc_open_checkpoint(v, testv, ct, n_lwe, checkpoint, len, &cp, &why)) {
        say("checkpoint: " + why);
        return VPBS_ERR_INVALID;
    }
    const unsigned k = cp.k;
    std::vector<u64>&words = cp.proof, &pis = cp.pis;
    steps = clamp_steps(steps, n_lwe);
    if (steps < k) {
        say("checkpoint: its counter " + std::to_string(k) + " is beyond the requested " + std::to_string(steps) + " steps");
        return VPBS_ERR_INVALID;
    }
    const double t_checks = now() - t0;
    // the key hash chain over the first k keys, beside the first resumed steps
    double t_keys = 0;
    bool keys_ok = false;
    std::thread key_chain([&] {
        name_thread("vpbs-resume-keys");
        const double t = now();
        keys_ok = vpbs::pbs_key_chain_prefix_matches(&pin, k, pis.data() + 2 * kn + 1);
        t_keys = now() - t;
    });
    long n_bytes;
    if (steps == k) {   // nothing to prove: the validated checkpoint itself
        n_bytes = len <= capacity ? (long)len : VPBS_ERR_INVALID;
        if (n_bytes > 0) std::memcpy(proof_out, checkpoint, len);
        else say("the output buffer is too small for the proof");
        if (timing) *timing = vpbs_ivc_timing{};
    } else {
        const ChainArgs a{v, testv, ct, bsk, ksk, n_lwe, k, words.data(), pis.data(), steps, proof_out, capacity, timing, err, err_len};
        n_bytes = v->dw_batch ? prove_pbs_device_witness(a) : prove_pbs_host(a);
    }
    key_chain.join();
    if (std::getenv("VPBS_TRACE_IVC"))
        std::fprintf(stderr, "[ivc resume] from step %u: parse + checks %.2f ms, key hash chain over %u keys %.3f s (beside the proof)\n", k, 1e3 * t_checks,
                     k, t_keys);
    if (!keys_ok) {   // the proof made from a checkpoint of other keys is discarded
        if (n_bytes > 0) std::memset(proof_out, 0, (size_t)n_bytes);
        say("checkpoint: the key hash chain does not match");
        return VPBS_ERR_INVALID;
    }
    if (n_bytes > 0 && timing) timing->seconds = now() - t0;
    return n_bytes;
}
}  // extern "C"

namespace vpbs {
void ivc_shape(const vpbs_ivc* v, IvcShape* out) {
    *out = IvcShape{v->N, v->K, v->cyc.log_n, v->kn, v->n_pi, v->cyc.n_preset, v->proof_words, v->ggsw_len, v->cyc.vk.size(),
                    v->cyc.vk.data(), v->dum.vk.data(), v->dummy_proof.data(), v->ctx};
}
bool ivc_open_checkpoint(const vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, unsigned n_lwe, const uint8_t* bytes, size_t len,
                         IvcCheckpoint* out, std::string* why) {
    if (!v || !testv || !ct || !bytes || !out || !why) {
        if (why) *why = "malformed arguments";
        return false;
    }
    const Side& cyc = v->cyc;
    const size_t n_pi = v->n_pi, cap_words = cyc.cs_cap.size();
    vpbs_compat compat;
    vpbs_ctx_get_compat(v->ctx, &compat);
    vpbs_verify_inputs vi{};   // the cyclic circuit as this object committed it: its own verifier data
    vi.log_n = cyc.log_n;
    vi.rate_bits = vpbs_ctx_rate_bits(v->ctx);
    vi.cap_height = vpbs_ctx_cap_height(v->ctx);
    vi.n_constants_sigmas = cyc.n_const_cols + cyc.n_routed;
    vi.n_wires = cyc.n_wires;
    vi.n_zs_partial_products = 20;
    vi.n_quotient = 16;
    vi.num_challenges = 2;
    vi.constants_sigmas_cap = cyc.cs_cap.data();
    for (int i = 0; i < 4; ++i) vi.circuit_digest[i] = cyc.vk[i];
    vi.n_constants = cyc.n_const_cols;
    vi.n_routed = cyc.n_routed;
    vi.quotient_degree_factor = 8;
    vi.gates = cyc.gates.data();
    vi.n_gates = (unsigned)cyc.gates.size();
    vi.num_selectors = cyc.num_selectors;
    vi.compat = &compat;
    const vpbs_verify_pbs_inputs pin{&vi, v->N, v->K, n_lwe, v->ggsw_len, testv, nullptr, ct, nullptr, nullptr};   // this form reads no keys
    char text[256] = {0};
    if (verify_pbs_prefix_without_keys(&pin, bytes, len, &out->k, text, sizeof text) != 1) {
        *why = text;
        return false;
    }
    // the proof words in target order (caps, openings, FRI) and the public inputs
    vpbs_step_inputs shape;
    vpbs_step_sizes sz{};
    cyc.step_inputs(shape, nullptr, true, nullptr);
    if (vpbs_step_sizes_get(v->ctx, &shape, &sz) != 0 || sz.cap_words != cap_words || 3 * sz.cap_words + sz.openings_words + sz.fri_words != v->proof_words) {
        *why = "the proof shape of this object is not the one its circuit expects";
        return false;
    }
    out->proof.assign(v->proof_words, 0);
    out->pis.assign(n_pi, 0);
    u64 *caps = out->proof.data(), *openings = caps + 3 * sz.cap_words, *fri = openings + sz.openings_words;
    if (vpbs_step_proof_from_bytes(&vi, bytes, len, caps, openings, fri, out->pis.data(), n_pi) != (long)n_pi) {
        *why = "the bytes are not a proof of this circuit (shape, canonical field elements, number of public inputs)";
        return false;
    }
    return true;
}

long ivc_prove_pbs_resident(vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, unsigned n_lwe, const IvcResidentChain* chain, unsigned from,
                            const uint64_t* from_proof, const uint64_t* from_pis, unsigned steps, uint8_t* proof_out, size_t capacity,
                            vpbs_ivc_timing* timing, char* err, size_t err_len) {
    report(err, err_len, "");
    if (!v || !testv || !ct || !chain || !chain->accs || !chain->key_links || !chain->lwe_links || !chain->fill || !proof_out || !v->dw_batch ||
        v->dw_late || v->cyc.comm || (from && (!from_proof || !from_pis))) {
        report(err, err_len, "malformed arguments (a resident chain needs the device-witness pipeline with the late phase on the host)");
        return VPBS_ERR_INVALID;
    }
    steps = clamp_steps(steps, n_lwe);
    if (from >= steps) {   // nothing to prove: the caller delivers the checkpoint itself
        report(err, err_len, "a resident chain from step `from` needs steps > from");
        return VPBS_ERR_INVALID;
    }
    v->ckpt_base = from;
    const long n = prove_pbs_device_witness({v, testv, ct, nullptr, nullptr, n_lwe, from, from_proof, from_pis, steps, proof_out, capacity, timing, err, err_len}, chain);
    v->ckpt_base = 0;
    return n;
}
}  // namespace vpbs

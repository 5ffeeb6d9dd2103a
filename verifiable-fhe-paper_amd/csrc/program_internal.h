// The seam between the program object (program.hip) and the five objects it drives: the Bootstrapper (pbs_batch.hip), the key ring
// (pbs_keyring.hip), the batch provers (pbs_prove_batch.hip, pbs_prove_ring.hip: two key sources of one worker pool, pbs_prove_pool.h, which
// holds the run both share) and the batch verifiers of whole vPBS proofs, one key set or a
// ring of key hashes (verify_pbs_batch.hip).  A program's ONE level walk queues one bootstrap launch per
// level behind its own combine kernel and waits once, at the end: it needs the launch of the Bootstrapper or of the key ring WITHOUT the
// wait their run ends with, and the shapes of objects whose structs are private to their files.  Its ONE proof check hands rows in
// device memory to the core that both statement verifiers hold, with the verifier's own key table.  Library-internal, like ivc_resident.h.
// The chain that the Bootstrapper's and the ring's kernels walk is one device function, pb_chain (pbs_chain.h); what the two objects share on
// the host -- shape, staging, thread rule, launch ladder, the run behind vpbs_*_run -- is pbs_chain_host.h.  The two enqueue functions below
// fill the object's own argument struct and go through that ladder.
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>

#include "../../include/vpbs_prover.h"

namespace vpbs {
struct DeviceError;
struct BootstrapperShape {
    vpbs_ctx* ctx;
    vpbs_tfhe_params prm;
    unsigned n_lwe;
    size_t max_batch;
};
void bootstrapper_shape(const vpbs_bootstrapper* b, BootstrapperShape* out);
// pbs_batch_kernel for `count` <= max_batch ciphertexts on device pointers, queued on the context's stream: the launch of
// vpbs_bootstrapper_run(.., on_device = 1) and nothing else -- no copy, no wait.  d_testv: [N], or [count][N] with testv_per_ct.  Any output
// may be null.  d_start [count] (device) with d_acc_in [count][K N]: the start mode of vpbs_bootstrapper_run_from, already checked; null: every
// row from step 0.  Throws vpbs::DeviceError (context.h) for a failed launch; the caller holds the device (hipSetDevice).
void bootstrapper_enqueue(vpbs_bootstrapper* b, const uint64_t* d_cts, size_t count, const uint64_t* d_testv, int testv_per_ct, uint64_t* d_out_ct,
                          uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start = nullptr, const uint64_t* d_acc_in = nullptr);
// Host-side check of the start steps of a run_from (both objects): true when every start[i] is at most n_lwe + 2 and acc_in is there for a row
// that needs it; else false with a message that names the row.  `who` is the entry point.
bool check_start_steps(const uint32_t* start, size_t count, unsigned n_lwe, const uint64_t* acc_in, const char* who, std::string* msg);
// the rows of a HOST acc_in [count][kn] with start[i] != 0 into d_acc_in, queued on the context's stream (rows with start 0 are not read)
void upload_acc_in(vpbs_ctx* ctx, uint64_t* d_acc_in, const uint64_t* acc_in, const uint32_t* start, size_t count, size_t kn);
// lwe_extract_kernel on device pointers, queued on `stream` (a hipStream_t): GLWEs [count][K][N] -> [count][n_lwe + 1]
void lwe_extract_enqueue(void* stream, const uint64_t* d_glwe, unsigned log_N, unsigned K, unsigned n_lwe, size_t count, uint64_t* d_lwe_out);
// lwe_extract_at_kernel (multi_lut.hip) on device pointers, queued on `stream`: row i of d_lwe_out [rows][n_lwe + 1] is the extraction of
// coefficient d_index[i] of GLWE d_src[i] of d_glwe [..][K][N]; nothing is checked; rows == 0 launches nothing
void lwe_extract_at_enqueue(void* stream, const uint64_t* d_glwe, const uint32_t* d_index, const uint32_t* d_src, unsigned log_N, unsigned K,
                            unsigned n_lwe, size_t rows, uint64_t* d_lwe_out);

// the batch prover's own Bootstrapper and the mutex that serialises its runs (vpbs_pbs_prover::boot_mu)
vpbs_bootstrapper* pbs_prover_bootstrapper(vpbs_pbs_prover* p, std::mutex** boot_mu);

// ---- the key ring (pbs_keyring.hip), for vpbs_program_run_batch ----
struct KeyringShape {
    vpbs_ctx* ctx;
    vpbs_tfhe_params prm;
    unsigned n_lwe;
    size_t max_keys, max_batch;
};
void keyring_shape(const vpbs_keyring* r, KeyringShape* out);
// the mutex that add, remove and run of the ring take: a caller that queues several launches holds it from its check of the slots to its wait
std::mutex& keyring_mutex(vpbs_keyring* r);
// Host-side check of key_of [count] against the ring's slots (the caller holds the mutex): true when every entry names a slot that holds
// a key set; else false, with vpbs_keyring_run's message in *msg -- `who` is the entry point, `what` the thing entry i stands for
// ("ciphertext", "instance").
bool keyring_check_slots(const vpbs_keyring* r, const uint32_t* key_of, size_t count, const char* who, const char* what, std::string* msg);
// pbs_keyring_kernel for `count` <= max_batch ciphertexts on device pointers, queued on the ring's context's stream: the launch of
// vpbs_keyring_run(.., on_device = 1) and nothing else -- no copy, no wait, no check.  d_order, d_key_of: [count] in device memory, as the
// kernel reads them (workgroup w handles ciphertext d_order[w] under slot d_key_of[d_order[w]]); they must stay unchanged until the launch
// has run.  d_testv: [N], or [count][N] with testv_per_ct.  Any output may be null.  Threads per ciphertext by the ring's rule.  Throws
// vpbs::DeviceError for a failed launch; the caller holds the mutex and the device (hipSetDevice).
void keyring_enqueue(vpbs_keyring* r, const uint64_t* d_cts, size_t count, const uint64_t* d_testv, int testv_per_ct, const uint32_t* d_order,
                     const uint32_t* d_key_of, uint64_t* d_out_ct, uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start = nullptr,
                     const uint64_t* d_acc_in = nullptr);   // d_start, d_acc_in: as bootstrapper_enqueue, indexed by ciphertext

// The device pointers the ring's table holds for `slot` (null for an empty slot or one out of range): what a prover of that slot's
// bootstraps reads the GGSW rows from.  The caller holds the ring's mutex, or otherwise knows that no add or remove is under way.
void keyring_slot_keys(const vpbs_keyring* r, unsigned slot, const uint64_t** d_bsk, const uint64_t** d_ksk);
// vpbs_keyring_add and vpbs_keyring_remove are these with owner = false.  After keyring_set_owned the ring refuses both with a message
// unless owner is true: the ring of a vpbs_ring_prover (pbs_prove_ring.hip), whose slots carry a key hash chain that the prover keeps.
void keyring_set_owned(vpbs_keyring* r);
int keyring_add(vpbs_keyring* r, const uint64_t* bsk, const uint64_t* ksk, int keys_on_device, unsigned* slot_out, bool owner);
int keyring_remove(vpbs_keyring* r, unsigned slot, bool owner);
// vpbs_keyring_add_seeded is this with owner = false: the key set expanded from mask_seed and its bodies (key_expand_device) into memory the
// ring owns, which keyring_remove frees as it frees what keyring_add uploaded; the slot number by keyring_add's rule
int keyring_add_seeded(vpbs_keyring* r, uint64_t mask_seed, const uint64_t* bsk_bodies, const uint64_t* ksk_bodies, int bodies_on_device,
                       unsigned* slot_out, bool owner);

// ---- seeded key sets (key_seeded.hip) ----
// the shapes vpbs_key_expand takes; false with the reason in *why
bool key_expand_shape_ok(const vpbs_tfhe_params* prm, unsigned n_lwe, std::string* why);
// The full keys in vpbs_keygen's layout at the DEVICE pointers d_bsk [n_lwe][K][ELL][K][N] and d_ksk [K][ELL][K][N] (16-byte aligned): the mask
// polynomials from mask_seed, the last polynomial of every GLWE from bsk_bodies [n_lwe][K][ELL][N] / ksk_bodies [K][ELL][N] (host arrays,
// uploaded for the call, or 16-byte aligned device pointers).  A pair (bodies, output) with a null member is skipped.  On the context's
// stream; returns after the wait.  Throws vpbs::DeviceError; the caller holds the device and whatever guards the context's pool.
void key_expand_device(vpbs_ctx* c, const vpbs_tfhe_params& prm, unsigned n_lwe, uint64_t mask_seed, const uint64_t* bsk_bodies,
                       const uint64_t* ksk_bodies, int bodies_on_device, uint64_t* d_bsk, uint64_t* d_ksk);

// ---- the ring prover (pbs_prove_ring.hip), for vpbs_program_prove_batch ----
// the mutex that add, remove and run of the ring prover take, and vpbs_ring_prover_run for a caller that holds it and has made the
// refusals of vpbs::ProvePool::check_run itself (count > 0): the check of the slots, then the pool's run
std::mutex& ring_prover_mutex(vpbs_ring_prover* p);
long ring_prover_run_locked(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                            unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len,
                            const uint8_t* const* checkpoints = nullptr, const size_t* lens = nullptr);   // checkpoints: vpbs_ring_prover_resume

struct PbsVerifierShape {
    vpbs_ctx* ctx;
    unsigned N, K, n_lwe;
    size_t max_batch;
};
void pbs_verifier_shape(const vpbs_pbs_verifier* v, PbsVerifierShape* out);

// ---- the core of both statement verifiers (verify_pbs_batch.hip), for vpbs_program_verify and vpbs_program_verify_batch ----
// Everything vpbs_pbs_verifier_run queues, on DEVICE pointers: ct [count][n_lwe + 1], out_ct [count][K N], a table of test vectors
// testvs [..][N] with testv_of [count], a table of key hashes [..][4] with key_of [count] -- proof i is checked against testvs[testv_of[i]]
// and key_hashes[key_of[i]]; digest and cap are the core's.  Queues the upload of the proof bytes (host memory), vp_lwe_chain (on the core's
// chain stream up to 64 proofs, on the context's stream above), the batch verifier's stages, the statement and vp_result on the context's
// stream, and leaves verdicts [count] | reasons [count] | proof reasons [count] in the core's result buffer: no wait after the upload.
// 1 <= count <= max_batch; the pointers must stay unchanged until pbs_verify_collect has returned.  Returns VPBS_OK, or VPBS_ERR_INVALID
// for offsets that decrease (nothing of the statement is queued then).  Throws vpbs::DeviceError; the caller holds the device.
struct PbsVerifyCore;
int pbs_verify_enqueue(PbsVerifyCore* c, const uint8_t* bytes, const size_t* offsets, size_t count, const uint64_t* d_ct, const uint64_t* d_out_ct,
                       const uint64_t* d_testvs, const uint32_t* d_testv_of, const uint64_t* d_key_hashes, const uint32_t* d_key_of);
// the read-back of what pbs_verify_enqueue left, and the one wait: the three bytes per proof into host arrays (reasons, proof_reasons may be
// null) -> the number of accepted proofs.  Throws vpbs::DeviceError.
long pbs_verify_collect(PbsVerifyCore* c, size_t count, uint8_t* verdicts, uint8_t* reasons, uint8_t* proof_reasons);
// after a DeviceError of either: the message into the context, the chain stream drained
void pbs_verify_abandon(PbsVerifyCore* c, const DeviceError& e);
// the core of a vpbs_pbs_verifier and its key table of one entry (device memory, [1][4]), for vpbs_program_verify
PbsVerifyCore* pbs_verifier_core(vpbs_pbs_verifier* v);
const uint64_t* pbs_verifier_key_table(const vpbs_pbs_verifier* v);

// ---- aggregation (aggregate.hip), for the program calls that end in one aggregate per instance ----
unsigned aggregator_levels(const vpbs_aggregator* a);     // up to 2^levels leaves
unsigned aggregator_device_witness(const vpbs_aggregator* a);   // max_nodes of vpbs_aggregator_set_device_witness (0: the host path)
size_t aggregator_max_bytes(const vpbs_aggregator* a);    // a capacity that holds the aggregate proof of every level
struct AggregateVerifierShape {
    vpbs_ctx* ctx;
    unsigned N, K, n_lwe, levels;   // levels: those the verifier has a batch verifier for
    size_t max_leaves, max_aggregates;
};
void aggregate_verifier_shape(const vpbs_aggregate_verifier* v, AggregateVerifierShape* out);

// ---- the ring verifier (verify_pbs_batch.hip) ----
struct RingVerifierShape {
    vpbs_ctx* ctx;
    unsigned N, K, n_lwe;
    size_t max_keys, max_batch;
};
void ring_verifier_shape(const vpbs_ring_verifier* v, RingVerifierShape* out);
// the mutex that set_key, clear_key and run take: a caller that queues several chunks holds it from its check of the slots to its last wait
std::mutex& ring_verifier_mutex(vpbs_ring_verifier* v);
PbsVerifyCore* ring_verifier_core(vpbs_ring_verifier* v);
const uint64_t* ring_verifier_key_table(const vpbs_ring_verifier* v);   // device memory, [max_keys][4]
// Host-side check of key_of [count] against the filled slots (the caller holds the mutex), in the key ring's wording: `who` is the entry
// point, `what` the thing entry i stands for ("proof", "instance").
bool ring_verifier_check_slots(const vpbs_ring_verifier* v, const uint32_t* key_of, size_t count, const char* who, const char* what,
                               std::string* msg);
}  // namespace vpbs

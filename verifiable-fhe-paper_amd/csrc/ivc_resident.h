// The seam between the IVC driver (ivc.hip), the device witness objects (witness_device.hip) and the batch prover (pbs_prove_batch.hip):
// a chain of the device-witness pipeline whose public inputs already exist -- accumulators from the Bootstrapper, the key hash chain of a
// resident key set, the chain's LWE hash links -- so that the driver computes none of them and uploads no preset matrix.  Library-internal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vpbs_prover.h"

namespace vpbs {
// what the batch prover needs to know of a vpbs_ivc (pointers stay valid while the object lives)
struct IvcShape {
    unsigned N, K, log_n;
    size_t kn, n_pi, n_preset, proof_words, ggsw_len, vk_words;
    const uint64_t *cyc_vk, *dum_vk, *dummy_proof;   // [vk_words], [vk_words], [proof_words]
    vpbs_ctx* ctx;
};
void ivc_shape(const vpbs_ivc* v, IvcShape* out);

// One chain's public inputs, where they already are.  `fill` queues, on `stream`, whatever writes the early-phase preset matrix
// [n_preset][cnt] (instances innermost) of chain steps [first, first + cnt) into d_matrix (device memory of the witness object's context);
// the device witness object runs its schedule behind it on the same stream.  Returns VPBS_OK or an error status.
struct IvcResidentChain {
    const uint64_t* accs;        // host [n_lwe + 2][K N]: the accumulator after every step
    const uint64_t* key_links;   // host [n_lwe + 2][4]: the key hash chain after every step
    const uint64_t* lwe_links;   // host [n_lwe + 2][4]: the LWE hash chain after every step
    int (*fill)(void* user, void* stream, unsigned first, unsigned cnt, uint64_t* d_matrix);
    void* user;
};
// vpbs_ivc_prove_pbs in the device-witness pipeline (vpbs_ivc_set_device_witness with batch > 0, late phase on the host) on such a chain: no
// native accumulator chain, no hashing of keys, no host-built preset matrix.  The same proofs, byte for byte.
// from > 0: the chain goes on at step `from` (vpbs_ivc_resume_pbs's way: no base proof, from_proof [proof_words] is step `from`'s inner proof
// and from_pis [n_pi] its predecessor's public inputs -- what ivc_open_checkpoint leaves).  accs, key_links and lwe_links stay indexed by
// ABSOLUTE chain step (entries below from - 1 are not read), and fill is called with absolute `first`.  from = 0: the proof pointers are not read.
long ivc_prove_pbs_resident(vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, unsigned n_lwe, const IvcResidentChain* chain, unsigned from,
                            const uint64_t* from_proof, const uint64_t* from_pis, unsigned steps, uint8_t* proof_out, size_t capacity,
                            vpbs_ivc_timing* timing, char* err, size_t err_len);

// A checkpoint opened against the object's own verifier data: the prefix form of vpbs_verify_pbs WITHOUT the key hash chain and without keys
// (claimed test vector, counter, the proof itself, its verifier data, the LWE hash chain over the first k masks of ct), then the proof words
// in target order (caps, openings, FRI) and the public inputs [acc_init | counter | accumulator | key hash | LWE hash | verifier data].
// Host only; reads the object, changes nothing: callers on several threads may share one object.  false with the verifier's text in `why`.
// The caller still owes the key hash: pis[2 K N + 1 .. + 4] against link k - 1 of the keys.
struct IvcCheckpoint {
    unsigned k = 0;
    std::vector<uint64_t> proof, pis;
};
bool ivc_open_checkpoint(const vpbs_ivc* v, const uint64_t* testv, const uint64_t* ct, unsigned n_lwe, const uint8_t* bytes, size_t len,
                         IvcCheckpoint* out, std::string* why);

// vpbs_witness_device_run on a preset matrix that `fill` leaves on the device: fill(user, stream, d_matrix) is called once, with the
// object's stream and a matrix of [n_preset][batch] words, before the schedule is queued
int witness_device_run_filled(vpbs_witness_device* d, unsigned batch, int (*fill)(void* user, void* stream, uint64_t* d_matrix), void* user);
}  // namespace vpbs

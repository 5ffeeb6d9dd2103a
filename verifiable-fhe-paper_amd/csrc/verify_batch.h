// The batch verifier of serialised step proofs (verify_batch.hip) as a routine other device verifiers build on: the vPBS statement verifier
// (verify_pbs_batch.hip) runs its stages and adds its own on the same stream.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vpbs_prover.h"

namespace vpbs {
// what a run leaves on the device, valid until the next run of the same verifier
struct ProofBatchView {
    const uint64_t* words;     // [count][W]: every proof's parsed words, its public inputs from n_fixed on (max_pi of them, zeros past its count)
    const uint32_t* n_pi;      // [count]: the public-input count each proof's bytes declare (0 where its length is malformed)
    const uint8_t* reasons;    // [count]: vpbs_verify_reason of each proof (VPBS_VERIFY_OK: accepted)
    uint32_t W, n_fixed, max_pi;
};
// Uploads the bytes and queues vb_parse .. vb_merkle and vb_result on the context's stream; waits for nothing after the upload.
// count >= 1.  Returns VPBS_OK, or VPBS_ERR_INVALID for count > max_batch, offsets that decrease or null pointers; throws DeviceError.
int proof_verifier_enqueue(vpbs_proof_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t count, ProofBatchView* view);
}  // namespace vpbs

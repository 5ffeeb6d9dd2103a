// Entries that exist for the test suite only: exported from the library, bound by api.py (INTERNAL_SIGNATURES), but NOT part of the C ABI
// of include/vpbs_prover.h and not in the Rust binding -- they may change or go without notice.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vpbs_prover.h"

extern "C" {
// The early-phase preset matrix of the device-witness pipeline as its host loop builds it (ivc.hip: preset_matrix_host): out
// [n_preset][count] (instances innermost, what vpbs_witness_device_run takes) for chain steps [first, first + count); pis [count][n_pi]: the
// public inputs of the PREDECESSORS of those steps.  Host only.  VPBS_ERR_INVALID for null pointers, count = 0 or first + count > n_lwe + 2.
int vpbs_test_ivc_preset_matrix(size_t proof_words, size_t n_pi, size_t ggsw_len, size_t vk_words, unsigned n_lwe, unsigned first, unsigned count,
                                const uint64_t* pis, const uint64_t* ct, const uint64_t* bsk, const uint64_t* ksk, const uint64_t* cyclic_vk,
                                const uint64_t* dummy_vk, const uint64_t* dummy_proof, uint64_t* out);
// The same matrix for the chain of one ciphertext, assembled on the device by the kernels of pbs_prove_pool.hip and copied to the host;
// preset_words: n_preset; dummy_proof: the [proof_words] dummy proof the object's vpbs_ivc holds on the host (the yardstick's constant).
int vpbs_test_pbs_prover_preset_matrix(vpbs_pbs_prover* p, const uint64_t* ct, const uint64_t* testv, unsigned first, unsigned count, uint64_t* out);
size_t vpbs_test_pbs_prover_preset_words(const vpbs_pbs_prover* p);
int vpbs_test_pbs_prover_dummy_proof(const vpbs_pbs_prover* p, uint64_t* out);
// What walk_step_proof (proof_shape.h) yields for the shape `in` describes (log_n, rate_bits, cap_height, the column counts, num_challenges,
// n_constants), as vpbs_proof_verifier_create records it (verify_batch.hip): src [*n_src] the byte offset of every word of the unified order
// caps | openings | fri in a serialised proof, lenb_off / lenb_val [*n_lenb] the offset and value of every Merkle-path length byte.  Returns
// the bytes up to and including the PoW witness.  Host only.  VPBS_ERR_INVALID for a null pointer, a shape vpbs_step_proof_from_bytes
// refuses or a capacity below the count (the counts are still written).  Tests bind it themselves: it has no entry in api.py.
// The preset matrix of a chunk of level-`level` nodes as the aggregator's device path assembles it (aggregate.hip: the upload of the child rows
// and ag_presets_kernel), copied to the host: rows [n_rows][row_words] the distinct child proofs, each flat | pis (row_words = the level's
// inner proof words + inner public inputs); pairs [batch][2] every node's (left row, right row); out [n_preset][batch], instances innermost.
// The aggregator's device witness must be on with max_nodes >= batch.  VPBS_ERR_INVALID for null pointers, a level the aggregator does not
// have, batch = 0 or above max_nodes, n_rows = 0 or above 2 batch, a pair entry at or above n_rows.
int vpbs_test_aggregator_preset_matrix(vpbs_aggregator* a, unsigned level, const uint64_t* rows, size_t n_rows, const uint32_t* pairs, unsigned batch,
                                       uint64_t* out);
// The streams the library holds on a device right now: out[0] the prover streams (one per open context, the witness contexts of a device
// pipeline included), out[1] the auxiliary ones (the device's shared upload stream once a vpbs_device_upload_bg has made it, and the gate-lane
// streams of contexts that ran with three gate lanes).  Touches no device.  VPBS_ERR_INVALID for a null pointer or a negative ordinal.
int vpbs_test_stream_counts(int device, unsigned out[2]);
long vpbs_test_proof_byte_tables(const vpbs_verify_inputs* in, size_t src_capacity, size_t lenb_capacity, uint32_t* src, uint32_t* lenb_off,
                                 uint8_t* lenb_val, size_t* n_src, size_t* n_lenb);
}

// The device witness checker (witness_check.hip) as the step prover uses it: the check of a step's device wires is queued on the prover's
// stream and its verdict travels to pinned memory behind the kernels, so that it arrives with the prover's next synchronisation (the read-back
// of the wires cap) instead of costing a round trip of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vpbs_prover.h"

namespace vpbs {
// true when the checker was made for a circuit of this shape on this context's device
bool witness_check_fits(const vpbs_witness_checker* chk, const vpbs_ctx* ctx, unsigned log_n, unsigned n_wires);
// queues the check of d_wires ([n_wires][n], device) on `s`; throws DeviceError when a launch fails
void witness_check_enqueue(vpbs_witness_checker* chk, hipStream_t s, const uint64_t* d_wires, const uint64_t pi_hash[4]);
// after `s` has been synchronised: true = satisfied; false: msg = vpbs_check_witness's message for the first violation
bool witness_check_result(const vpbs_witness_checker* chk, std::string& msg);
}  // namespace vpbs

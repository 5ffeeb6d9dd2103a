// Rotation margins: what a bootstrap will look up, from the ciphertext and the LWE key alone, stated once for host and
// device.  The chain (pb_chain, pbs_chain.h) never rounds the PHASE of its input: it mod-switches every word by itself (pb_mod_switch),
// after the snap for a multi-output gate (multi_lut::snap), and rotates the test vector by the sum of those rounded words.  For a row ct of
// n + 1 words and a key s of n words, each 0 or 1, with L = log_N + 1:
//   w_i  = snap(ct[i], log_N, log_slots)                      (log_slots = 0: the reduced word; a snapped word is a fixed point)
//   R    = (ms(neg(w_n)) + sum over i < n with s_i = 1 of ms(w_i)) mod 2N        step 0 and the n CMUX steps of pb_chain
//   mu   = (2N - R) mod 2N
// PREDICTION CONTRACT: with noise-free keys and an exact decomposition, coefficient j of the phase of the bootstrap's output GLWE under
// test vector testv is E(mu + j), indices mod 2N: E(x) = testv[x] for x < N, neg(testv[x - N]) otherwise (pb_rotated_coeff read at mu + j).
// With the p of vpbs_lut_testv, block = N / p and h = block / 2:
//   idx  = ((mu + h) / block) mod 2p        the table position the bootstrap reads; positions [p, 2p) are the negated half
//   ref  = expected mod 2p when expected is given, else idx
//   dev  = (mu - ref * block) mod 2N, centred into [-N, N)
//   failure: expected given and idx != ref
// Everything is below 2^18, so u32 sums are exact: 2N divides 2^32.
#pragma once
#include "gl.h"
#include "multi_lut.h"
#include "pbs_chain.h"

namespace vpbs {
namespace rotation {
using gl::u64;

// the rotation one word contributes: ms(w) for a mask word (when its key bit is 1), ms(neg(w)) for the body
GL_HD unsigned word_rotation(u64 word, unsigned log_n, unsigned log_slots, bool body) {
    const u64 w = multi_lut::snap(word, log_n, log_slots);
    return pb_mod_switch(body ? gl::neg(w) : w, log_n);
}

struct Margin {
    unsigned mu, idx, abs;   // abs = |dev| <= N
    bool neg, fail;
};
// from the sum of the word rotations (any representative mod 2N)
GL_HD Margin margin(unsigned rotation_sum, unsigned log_n, unsigned p, bool has_expected, u64 expected) {
    const unsigned n = 1u << log_n, two_n = 2 * n, block = n / p, h = block / 2;
    Margin m;
    m.mu = (two_n - (rotation_sum & (two_n - 1))) & (two_n - 1);
    m.idx = ((m.mu + h) / block) & (2 * p - 1);
    const unsigned ref = has_expected ? (unsigned)(expected & (2 * p - 1)) : m.idx;
    const unsigned d = (m.mu + two_n - ref * block) & (two_n - 1);   // ref * block < 2N
    m.neg = d >= n;
    m.abs = m.neg ? two_n - d : d;
    m.fail = has_expected && m.idx != ref;
    return m;
}
}  // namespace rotation
}  // namespace vpbs

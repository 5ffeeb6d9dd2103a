// Multi-output lookup gates: the two word-level functions that the primitives (multi_lut.hip) and the program object
// (program.hip) share, stated once for host and device.
//   snap      rounds a ciphertext word to a multiple of 2^t, t = 64 - log2(2N) + slots_log: the mod switch of the step circuit
//             (pb_mod_switch, pbs_chain.h) then gives a rotation that is a multiple of 2^slots_log for every word, and so for their sum.
//   extract_at  word c of the sample extraction of coefficient j of a GLWE: the LWE ciphertext under the flattened GLWE key whose phase is
//             coefficient j of the GLWE's phase.
#pragma once
#include "gl.h"

namespace vpbs {
namespace multi_lut {
using gl::u64;

// slots_log = 0: the reduced word, no rounding.  Otherwise r = (w >> t) + bit t - 1 of w, result (r << t) mod 2^64: a multiple of 2^t with
// t >= 32 for log_N <= 31, hence below p = 2^64 - 2^32 + 1; r = 2^(64 - t) wraps to 0.
GL_HD u64 snap(u64 word, unsigned log_n, unsigned slots_log) {
    const u64 w = gl::canon(word);
    if (slots_log == 0) return w;
    const unsigned t = 64 - (log_n + 1) + slots_log;   // 1 <= slots_log <= log_n: 64 - log_n <= t <= 63
    const u64 r = (w >> t) + ((w >> (t - 1)) & 1);
    return r >> (64 - t) ? 0 : r << t;
}

// word c < n_lwe of the extraction at coefficient j: over mask polynomial a = ct[c / N], full[c'] = a[j - c'] for c' <= j, else
// -a[N + j - c'] (in the field: 0 stays 0); word n_lwe is body[j]
GL_HD u64 extract_at_word(const u64* ct, unsigned log_n, unsigned K, unsigned n_lwe, unsigned j, unsigned c) {
    const unsigned n = 1u << log_n;
    if (c == n_lwe) return ct[(size_t)(K - 1) * n + j];
    const unsigned poly = c >> log_n, cc = c & (n - 1);
    const u64* a = ct + (size_t)poly * n;
    return cc <= j ? a[j - cc] : gl::neg(a[n + j - cc]);
}
}  // namespace multi_lut
}  // namespace vpbs

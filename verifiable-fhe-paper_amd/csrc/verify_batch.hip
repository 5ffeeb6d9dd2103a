// Batch verifier of serialised step proofs on the device: vpbs_step_proof_from_bytes + vpbs_verify_step (verifier.hip) for many
// ProofWithPublicInputs byte strings at once, with the host's verdict for every one of them.  The two verifiers share what a verdict rests
// on: the proof's shape, the refusal rules and the serialised order (proof_shape.h), the vanishing identity and the arithmetic of a FRI
// query (verify_core.h).  This file owns how the work is spread over lanes: the gather, the 16-lane challenger, the per-gate evaluation,
// the Merkle climbs and the flags.
//
// Layout (made once, at vpbs_proof_verifier_create, from the circuit's shape):
//   src   [n_fixed]: for every word of a proof in the unified order caps [3][cap] | openings | fri, its byte offset in the serialised
//                    proof -- walk_step_proof, recorded once;
//   lenb  [..]:      byte offset and expected value of every Merkle-path length byte;
//   the constants/sigmas cap, the gates and the CosetTables of gates::coset_tables.
// Per proof the device keeps its words (stride W: the fixed words, then max_public_inputs public inputs), a challenge block and a flag word.
//
// Stages, one kernel each, handing off at kernel boundaries:
//   vb_parse      one lane per word: unaligned gather from the raw bytes, canonicity, path-length bytes, public-input count   -> MALFORMED
//   vb_transcript one 16-lane group per proof (poseidon::permute_wide): public-input hash, the challenger of vpbs_verify_step, PoW
//                 check, the query indices                                                                                    -> POW
//   vb_gates      one lane per (proof, gate): the gates.h evaluators over GF(p^2) at zeta, filtered and folded with the alphas
//   vb_vanishing  one lane per proof: the gate terms + the permutation / partial-product terms == Z_H(zeta) t(zeta)          -> VANISHING
//   vb_fri        one lane per (proof, query): fri_combine_initial, the folds and the final polynomial                         -> FRI
//   vb_merkle     one lane per (proof, path): leaf hash_or_noop and the climb to the cap                                       -> MERKLE
//   vb_result     the flags to one verdict and one reason per proof: the first failing check in the host's order.
// Every stage runs on every proof, whatever an earlier stage found; the result kernel orders the findings.  A proof's stages read only
// its own words (a failed parse leaves zeros or the raw words in them, never memory outside the proof), so no proof affects another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host/plonky2_mirror.h"
#include "gl.h"
#include "poseidon.h"
#include "gates.h"
#include "context.h"
#include "proof_shape.h"
#include "test_entries.h"
#include "verify_batch.h"
#include "verify_core.h"

namespace {
using vpbs::DeviceError;
using vpbs::report;
using gl::Ext;
using u32 = uint32_t;
using u64 = uint64_t;

constexpr u32 F_MALFORMED = 1, F_VANISHING = 2, F_POW = 4, F_FRI = 8, F_MERKLE = 16;
constexpr unsigned NC_MAX = 4;        // challenges per proof the device path carries in registers
constexpr unsigned MAX_BATCH = 65535;

// the shape every kernel reads (passed by value): the proof's, and the slots the device keeps per proof
struct Shape : vpbs::ProofShape {
    u32 W;                        // words per proof: n_fixed, then max_pi public inputs
    u32 n_lenb, max_pi;
    u32 CH;                       // words of a challenge block
    u64 digest[4];
};
// challenge block: pih [4] | betas | gammas | alphas [nc] | zeta [2] | fri_alpha [2] | fri_betas [n_rounds][2] | x_index [nq]
__host__ __device__ inline u32 ch_betas(const Shape&) { return 4; }
__host__ __device__ inline u32 ch_gammas(const Shape& s) { return 4 + s.nc; }
__host__ __device__ inline u32 ch_alphas(const Shape& s) { return 4 + 2 * s.nc; }
__host__ __device__ inline u32 ch_zeta(const Shape& s) { return 4 + 3 * s.nc; }
__host__ __device__ inline u32 ch_fri_alpha(const Shape& s) { return 6 + 3 * s.nc; }
__host__ __device__ inline u32 ch_fri_betas(const Shape& s) { return 8 + 3 * s.nc; }
__host__ __device__ inline u32 ch_xq(const Shape& s) { return 8 + 3 * s.nc + 2 * s.n_rounds; }

__device__ __forceinline__ u64 load_unaligned(const u64* base, u64 byte) {
    const u64 k = byte >> 3;
    const unsigned sh = (unsigned)(byte & 7) * 8;
    const u64 lo = base[k];
    return sh ? (lo >> sh) | (base[k + 1] << (64 - sh)) : lo;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// parse: grid (words / 256, proofs).  raw: the batch's bytes from offset 0 (8-aligned, 16 bytes of padding behind), offs [count + 1]
__device__ bool pi_count(const u64* raw, u64 start, u64 len, const Shape& S, u64& n_pi) {
    n_pi = 0;
    if (len < S.fixed_len) return false;
    if (!S.pi_prefix) {
        if ((len - S.fixed_len) % 8) return false;
        n_pi = (len - S.fixed_len) / 8;
        return n_pi <= S.max_pi;
    }
    if (len < (u64)S.fixed_len + 8) return false;
    n_pi = load_unaligned(raw, start + S.fixed_len);
    if (n_pi > S.max_pi) return false;
    return len == (u64)S.fixed_len + 8 + 8 * n_pi;
}

__global__ __launch_bounds__(256) void vb_parse(const u64* __restrict__ raw, const u64* __restrict__ offs, const u32* __restrict__ src,
                                                const u32* __restrict__ lenb_off, const uint8_t* __restrict__ lenb_val, Shape S,
                                                u64* __restrict__ words, u32* __restrict__ n_pi_out, u32* __restrict__ flags) {
    const u32 i = blockIdx.y;
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    const u64 start = offs[i], len = offs[i + 1] - offs[i];
    u64* w = words + (u64)i * S.W;
    bool bad = false;
    if (j < S.n_fixed) {
        const u64 b = src[j];
        u64 v = 0;
        if (b + 8 <= len) {
            v = load_unaligned(raw, start + b);
            if (v >= gl::P && j != S.o_fri + S.fri_total - 1) bad = true;   // the PoW witness is a plain u64 to the parser
        } else {
            bad = true;
        }
        w[j] = v;
    } else if (j < S.n_fixed + S.max_pi) {
        u64 n_pi;
        const bool ok = pi_count(raw, start, len, S, n_pi);
        const u32 k = j - S.n_fixed;
        u64 v = 0;
        if (ok && k < n_pi) {
            v = load_unaligned(raw, start + S.fixed_len + (S.pi_prefix ? 8 : 0) + 8 * (u64)k);
            if (v >= gl::P) bad = true;
        }
        w[j] = v;
    }
    if (j == 0) {   // the length and public-input count: lane 0 always exists (n_fixed >= 1), whatever max_public_inputs is
        u64 n_pi;
        const bool ok = pi_count(raw, start, len, S, n_pi);
        if (!ok) bad = true;
        n_pi_out[i] = ok ? (u32)n_pi : 0;
    }
    if (j < S.n_lenb) {
        const u64 b = lenb_off[j];
        if (b >= len || ((raw[(start + b) >> 3] >> (8 * ((start + b) & 7))) & 0xFF) != lenb_val[j]) bad = true;
    }
    if (bad) atomicOr(&flags[i], F_MALFORMED);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// transcript: one proof per 16-lane block; lane l < 12 owns sponge element l (the permute_wide layout).  Every lane runs the same control
// flow; `out` holds the 12 words of the state after the last permutation (the challenger's output buffer is out[0..8)).
__device__ __noinline__ u64 perm16(u64 x, u64* sh, u64* out, unsigned l) {
    x = poseidon::permute_wide(x, sh, l);
    __syncthreads();
    if (l < 12) out[l] = x;
    __syncthreads();
    return x;
}

struct Challenger16 {
    u64 x = 0;
    unsigned in_len = 0, out_len = 0, l;
    u64 *sh, *out;
    __device__ void duplex() {   // overwrite mode: the observed elements were written into the state as they came
        in_len = 0;
        x = perm16(x, sh, out, l);
        out_len = 8;
    }
    __device__ void observe(u64 e) {
        out_len = 0;
        if (l == in_len) x = e;
        if (++in_len == 8) duplex();
    }
    __device__ u64 get() {
        if (in_len != 0 || out_len == 0) duplex();
        return out[--out_len];
    }
};

__global__ __launch_bounds__(16) void vb_transcript(const u64* __restrict__ words, const u32* __restrict__ n_pi, Shape S, u64* __restrict__ chal, u32* __restrict__ flags) {
    __shared__ u64 sh[poseidon::WIDE_LDS_WORDS];
    __shared__ u64 out[16];
    const unsigned l = threadIdx.x;
    const u32 i = blockIdx.x;
    const u64* w = words + (u64)i * S.W;
    u64* ch = chal + (u64)i * S.CH;
    out[l] = 0;
    __syncthreads();
    // hash_no_pad of the public inputs
    {
        const u32 npi = min(n_pi[i], S.max_pi);   // vb_parse writes at most max_pi; the bound keeps the reads inside the proof's slot
        u64 x = 0;
        for (u32 off = 0; off < npi; off += 8) {
            const u32 len = npi - off < 8 ? npi - off : 8;
            if (l < len) x = w[S.n_fixed + off + l];
            x = perm16(x, sh, out, l);
        }
    }
    u64 pih[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pih[k] = out[k];
    __syncthreads();
    Challenger16 c;
    c.l = l;
    c.sh = sh;
    c.out = out;
    for (int k = 0; k < 4; ++k) c.observe(S.digest[k]);
    for (int k = 0; k < 4; ++k) c.observe(pih[k]);
    for (u32 k = 0; k < S.cap_words; ++k) c.observe(w[k]);
    u64 v;
    for (u32 a = 0; a < S.nc; ++a) { v = c.get(); if (l == 0) ch[ch_betas(S) + a] = v; }
    for (u32 a = 0; a < S.nc; ++a) { v = c.get(); if (l == 0) ch[ch_gammas(S) + a] = v; }
    for (u32 k = 0; k < S.cap_words; ++k) c.observe(w[S.cap_words + k]);
    for (u32 a = 0; a < S.nc; ++a) { v = c.get(); if (l == 0) ch[ch_alphas(S) + a] = v; }
    for (u32 k = 0; k < S.cap_words; ++k) c.observe(w[2 * S.cap_words + k]);
    for (u32 k = 0; k < 2; ++k) { v = c.get(); if (l == 0) ch[ch_zeta(S) + k] = v; }
    for (u32 k = 0; k < S.n_open_words; ++k) c.observe(w[S.o_open + k]);
    for (u32 k = 0; k < 2; ++k) { v = c.get(); if (l == 0) ch[ch_fri_alpha(S) + k] = v; }
    for (u32 r = 0; r < S.n_rounds; ++r) {
        for (u32 k = 0; k < S.cap_words; ++k) c.observe(w[S.o_fri + r * S.cap_words + k]);
        for (u32 k = 0; k < 2; ++k) { v = c.get(); if (l == 0) ch[ch_fri_betas(S) + 2 * r + k] = v; }
    }
    const u64* fin = w + S.o_fri + S.fri_total - 1 - 2 * S.final_len;
    for (u32 k = 0; k < 2 * S.final_len; ++k) c.observe(fin[k]);
    const u64 pow = w[S.o_fri + S.fri_total - 1];
    bool pow_bad = pow >= gl::P;
    c.observe(pow);
    const u64 resp = c.get();
    if (S.pow_bits && (resp >> (64 - S.pow_bits)) != 0) pow_bad = true;
    const u64 lde_mask = ((u64)1 << S.log_lde) - 1;
    for (u32 q = 0; q < S.nq; ++q) { v = c.get(); if (l == 0) ch[ch_xq(S) + q] = v & lde_mask; }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ch[k] = pih[k];
        if (pow_bad) atomicOr(&flags[i], F_POW);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// gate constraints at zeta: grid (proofs / 64, gates) -- one gate per block, so the dispatch is uniform
struct DevVars {
    const u64* wires;       // [n_wires][2]
    const u64* constants;   // first gate constant, [..][2]
    unsigned n_wires, n_constants;
    const u64* pih;
    __device__ Ext wire(unsigned i) const { return i < n_wires ? Ext{wires[2 * i], wires[2 * i + 1]} : gl::ext(0); }
    __device__ Ext constant(unsigned i) const { return i < n_constants ? Ext{constants[2 * i], constants[2 * i + 1]} : gl::ext(0); }
    __device__ u64 pi_hash(unsigned i) const { return pih[i]; }
};
// sum_k alpha_a^k c_k as the constraints arrive: the host's total[k] folded with the powers of alpha (the sum over gates is linear)
struct AlphaSink {
    unsigned nc;
    u64 alpha[NC_MAX];
    Ext apow[NC_MAX], acc[NC_MAX];
    __device__ void push(Ext x) {
#pragma unroll
        for (unsigned a = 0; a < NC_MAX; ++a)
            if (a < nc) {
                acc[a] = gl::add(acc[a], gl::mul(apow[a], x));
                apow[a] = gl::mul(apow[a], alpha[a]);
            }
    }
};

__global__ __launch_bounds__(64) void vb_gates(const u64* __restrict__ words, const u64* __restrict__ chal, const vpbs_gate* __restrict__ gate_list,
                                               const gates::CosetTables* __restrict__ coset, Shape S, u32 count, u64* __restrict__ gterms) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    const u32 gi = blockIdx.y;
    if (i >= count) return;
    const u64* open = words + (u64)i * S.W + S.o_open;
    const u64* ch = chal + (u64)i * S.CH;
    const vpbs_gate g = gate_list[gi];
    const DevVars v{open + 2 * (u64)S.ncols[0], open + 2 * (u64)S.num_selectors, S.ncols[1], S.n_constants - S.num_selectors, ch};
    AlphaSink s;
    s.nc = S.nc;
#pragma unroll
    for (unsigned a = 0; a < NC_MAX; ++a) {
        s.alpha[a] = a < S.nc ? ch[ch_alphas(S) + a] : 0;
        s.apow[a] = gl::ext(1);
        s.acc[a] = gl::ext(0);
    }
    gates::eval_gate<Ext>(g, &coset[g.p0 <= 5 ? g.p0 : 0], v, s);
    const Ext sel{open[2 * (u64)g.selector_index], open[2 * (u64)g.selector_index + 1]};
    const Ext filter = gates::compute_filter<Ext>(g, sel, S.num_selectors > 1);
    u64* o = gterms + ((u64)i * S.n_gates + gi) * 2 * S.nc;
    for (unsigned a = 0; a < S.nc && a < NC_MAX; ++a) {
        const Ext t = gl::mul(filter, s.acc[a]);
        o[2 * a] = t.c0;
        o[2 * a + 1] = t.c1;
    }
}

// the vanishing identity at zeta: one lane per proof, the gate terms of a challenge summed over the per-gate partials of vb_gates
__global__ __launch_bounds__(64) void vb_vanishing(const u64* __restrict__ words, const u64* __restrict__ chal, const u64* __restrict__ gterms,
                                                   Shape S, u32 count, u32* __restrict__ flags) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const u64* open = words + (u64)i * S.W + S.o_open;
    const u64* ch = chal + (u64)i * S.CH;
    const Ext zeta = vpbs::ext_at(ch + ch_zeta(S), 0);
    const vpbs::ZetaTerms zt = vpbs::zeta_terms(S, zeta);
    bool ok = true;
    for (unsigned a = 0; a < S.nc; ++a) {
        const auto gate_term = [&] {   // the sum over the per-gate partials of vb_gates: [proof][gate][challenge][2]
            Ext gt = gl::ext(0);
            const u64* t = gterms + (u64)i * S.n_gates * 2 * S.nc;
            for (unsigned g = 0; g < S.n_gates; ++g) gt = gl::add(gt, vpbs::ext_at(t + (u64)g * 2 * S.nc, a));
            return gt;
        };
        if (!vpbs::vanishing_holds(S, open, a, ch[ch_alphas(S) + a], ch + ch_betas(S), zeta, zt, gate_term)) ok = false;
    }
    if (!ok) atomicOr(&flags[i], F_VANISHING);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// FRI query rounds: one lane per (proof, query)
__global__ __launch_bounds__(64) void vb_fri(const u64* __restrict__ words, const u64* __restrict__ chal, Shape S, u32 count,
                                             u32* __restrict__ flags) {
    const u64 t = (u64)blockIdx.x * 64 + threadIdx.x;
    if (t >= (u64)count * S.nq) return;
    const u32 i = (u32)(t / S.nq), q = (u32)(t % S.nq);
    const u64* w = words + (u64)i * S.W;
    const u64* ch = chal + (u64)i * S.CH;
    const Ext zeta = vpbs::ext_at(ch + ch_zeta(S), 0), fri_alpha = vpbs::ext_at(ch + ch_fri_alpha(S), 0);
    Ext reduced0, reduced1;
    vpbs::reduced_openings(S, w + S.o_open, fri_alpha, reduced0, reduced1);
    const u64* qw = w + S.o_fri + S.o_queries + (u64)q * S.query_words;
    const u64* fin = w + S.o_fri + S.fri_total - 1 - 2 * S.final_len;
    if (!vpbs::fri_query_holds(S, reduced0, reduced1, qw, fin, (u32)ch[ch_xq(S) + q], zeta, fri_alpha, ch + ch_fri_betas(S)))
        atomicOr(&flags[i], F_FRI);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Merkle paths: one lane per (proof, path); paths of a query: the 4 initial oracles, then one per reduction round
__global__ __launch_bounds__(64) void vb_merkle(const u64* __restrict__ words, const u64* __restrict__ chal, const u64* __restrict__ cs_cap,
                                                Shape S, u32 count, u32* __restrict__ flags) {
    const u32 per_q = 4 + S.n_rounds;
    const u64 t = (u64)blockIdx.x * 64 + threadIdx.x;
    if (t >= (u64)count * S.nq * per_q) return;
    const u32 i = (u32)(t / (S.nq * per_q));
    const u32 rem = (u32)(t % (S.nq * per_q));
    const u32 q = rem / per_q, o = rem % per_q;
    const u64* w = words + (u64)i * S.W;
    const u64* qw = w + S.o_fri + S.o_queries + (u64)q * S.query_words;
    u32 idx = (u32)chal[(u64)i * S.CH + ch_xq(S) + q];
    const u64 *leaf, *cap;
    u32 leaf_len, nsib;
    if (o < 4) {
        leaf = qw + S.off_o[o];
        leaf_len = S.ncols[o];
        nsib = S.nsib0;
        cap = o == 0 ? cs_cap : w + (u64)(o - 1) * S.cap_words;
    } else {
        const u32 r = o - 4;
        for (u32 k = 0; k <= r; ++k) idx >>= S.ab[k];
        leaf = qw + S.off_r[r];
        leaf_len = 2u << S.ab[r];
        nsib = S.nsib_r[r];
        cap = w + S.o_fri + (u64)r * S.cap_words;
    }
    const u64* sib = leaf + leaf_len;
    u64 s[12];
    u64 cur[4];
    if (leaf_len <= 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = (u32)k < leaf_len ? leaf[k] : 0;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = 0;
        for (u32 off = 0; off < leaf_len; off += 8) {
            const u32 len = leaf_len - off < 8 ? leaf_len - off : 8;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if ((u32)k < len) s[k] = leaf[off + k];
            poseidon::permute(s);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = s[k];
    }
    for (u32 k = 0; k < nsib; ++k) {
        const bool right = idx & 1;   // this node is the right child: two_to_one(sibling, node)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const u64 sv = sib[4 * k + e];
            s[e] = right ? sv : cur[e];
            s[e + 4] = right ? cur[e] : sv;
            s[e + 8] = 0;
        }
        poseidon::permute(s);
#pragma unroll
        for (int e = 0; e < 4; ++e) cur[e] = s[e];
        idx >>= 1;
    }
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && cur[e] == cap[4 * (u64)idx + e];
    if (!ok) atomicOr(&flags[i], F_MERKLE);
}

// the first failing check in the host verifier's order: parse, vanishing identity, PoW, FRI, Merkle paths
__global__ __launch_bounds__(256) void vb_result(const u32* __restrict__ flags, u32 count, uint8_t* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u32 f = flags[i];
    const uint8_t reason = (f & F_MALFORMED) ? VPBS_VERIFY_MALFORMED
                           : (f & F_VANISHING) ? VPBS_VERIFY_VANISHING
                           : (f & F_POW)       ? VPBS_VERIFY_POW
                           : (f & F_FRI)       ? VPBS_VERIFY_FRI
                           : (f & F_MERKLE)    ? VPBS_VERIFY_MERKLE
                                               : VPBS_VERIFY_OK;
    out[i] = reason == VPBS_VERIFY_OK ? 1 : 0;
    out[count + i] = reason;
}

// walk_step_proof, recorded once: for every word of the unified order its byte offset in a serialised proof, and the offset and expected
// value of every Merkle-path length byte
struct ByteTables {
    std::vector<u32> src, lenb_off;
    std::vector<uint8_t> lenb_val;
    size_t pos = 0, n_words = 0;
    void words(u32 dest, size_t cnt, bool) {
        for (size_t k = 0; k < cnt; ++k) src[dest + k] = (u32)(pos + 8 * k);
        pos += 8 * cnt;
        n_words += cnt;
    }
    void length_byte(unsigned nsib) {
        lenb_off.push_back((u32)pos);
        lenb_val.push_back((uint8_t)nsib);
        ++pos;
    }
    const char* record(const vpbs::ProofShape& S) {   // -> NULL, or which self-check of the layout failed
        src.assign(S.n_fixed, ~0u);
        vpbs::walk_step_proof(S, *this);
        plonky2::FriParams fp = plonky2::FriParams::standard(S.log_n, S.rate_bits, S.cap_height);
        if (n_words != S.n_fixed || pos != S.fixed_len || S.fri_total != plonky2::fri_proof_words(fp, {S.ncols[0], S.ncols[1], S.ncols[2], S.ncols[3]}))
            return "proof layout does not match the FRI proof size";
        for (u32 s : src)
            if (s == ~0u) return "proof layout leaves a word unset";
        return nullptr;
    }
};
}  // namespace

struct vpbs_proof_verifier {
    vpbs_ctx* ctx = nullptr;
    Shape S{};
    size_t max_batch = 0;
    u64 *d_words = nullptr, *d_chal = nullptr, *d_gterms = nullptr, *d_cs_cap = nullptr;
    u32 *d_src = nullptr, *d_lenb_off = nullptr, *d_npi = nullptr, *d_flags = nullptr;
    uint8_t *d_lenb_val = nullptr, *d_out = nullptr;
    vpbs_gate* d_gates = nullptr;
    gates::CosetTables* d_coset = nullptr;
    u64* d_stage = nullptr;           // offsets [count + 1] | raw bytes | padding, as one upload
    size_t stage_bytes = 0;
    uint8_t* h_stage = nullptr;       // pinned
    size_t h_stage_bytes = 0;
    std::vector<void*> owned;

    template <class T> T* alloc(size_t count) {
        T* d = static_cast<T*>(ctx->alloc_bytes(std::max<size_t>(1, count) * sizeof(T)));
        owned.push_back(d);
        return d;
    }
    template <class T> T* upload(const T* h, size_t count) {
        T* d = alloc<T>(count);
        if (count) VPBS_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return d;
    }
    ~vpbs_proof_verifier() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
        if (d_stage) ctx->release(d_stage);
        if (h_stage) (void)hipHostFree(h_stage);
    }
};

extern "C" {
int vpbs_proof_verifier_create(vpbs_ctx* ctx, const vpbs_verify_inputs* in, size_t max_batch, size_t max_public_inputs,
                               vpbs_proof_verifier** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    auto refuse = [&](const char* m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !in || !out || !in->constants_sigmas_cap) return refuse("null argument");
    if (max_batch == 0 || max_batch > MAX_BATCH) return refuse("max_batch must be 1 .. 65535");
    if (max_public_inputs > (1u << 24)) return refuse("max_public_inputs above 2^24");
    // what vpbs_step_proof_from_bytes and vpbs_verify_step refuse.  The device's own two limits go in as a callback and not in front of the
    // call on purpose: a description that breaks several rules is then refused with the message this entry has always given first
    Shape S{};
    std::string why;
    const bool fits = vpbs::make_proof_shape(*in, vpbs::compat_of(*in), vpbs::SHAPE_PARSE | vpbs::SHAPE_VERIFY, S, &why, [&]() -> const char* {
        if (in->num_challenges > NC_MAX) return "the device verifier carries at most 4 challenges";
        if (in->gate_terms_zeta && !(in->gates && in->n_gates)) return "gate_terms_zeta without gates: a batch of proofs has one zeta per proof";
        return nullptr;
    });
    if (!fits) return refuse(why.c_str());
    ByteTables tab;
    if (const char* m = tab.record(S)) return refuse(m);
    const size_t cap_words = S.cap_words, nc = S.nc;

    S.max_pi = (u32)max_public_inputs;
    S.W = (u32)((S.n_fixed + max_public_inputs + 1) & ~(size_t)1);
    S.n_lenb = (u32)tab.lenb_off.size();
    S.CH = (u32)(8 + 3 * nc + 2 * S.n_rounds + S.nq);
    for (int k = 0; k < 4; ++k) S.digest[k] = in->circuit_digest[k];

    auto* v = new vpbs_proof_verifier;
    v->ctx = ctx;
    v->S = S;
    v->max_batch = max_batch;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        v->d_src = v->upload(tab.src.data(), tab.src.size());
        v->d_lenb_off = v->upload(tab.lenb_off.data(), tab.lenb_off.size());
        v->d_lenb_val = v->upload(tab.lenb_val.data(), tab.lenb_val.size());
        v->d_cs_cap = v->upload(in->constants_sigmas_cap, cap_words);
        if (S.n_gates) {
            v->d_gates = v->upload(in->gates, in->n_gates);
            gates::CosetTables t[6];
            for (unsigned b = 0; b < 6; ++b) t[b] = gates::coset_tables(b);
            v->d_coset = v->upload(t, 6);
            v->d_gterms = v->alloc<u64>(max_batch * S.n_gates * 2 * nc);
        }
        v->d_words = v->alloc<u64>(max_batch * (size_t)S.W);
        v->d_chal = v->alloc<u64>(max_batch * (size_t)S.CH);
        v->d_npi = v->alloc<u32>(max_batch);
        v->d_flags = v->alloc<u32>(max_batch);
        v->d_out = v->alloc<uint8_t>(2 * max_batch);
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // the host vectors above go out of scope
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        delete v;
        return e.status;
    }
    *out = v;
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_proof_verifier_free(vpbs_proof_verifier* v) { delete v; }
}  // extern "C"

int vpbs::proof_verifier_enqueue(vpbs_proof_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t count, ProofBatchView* view) {
    if (!v || !bytes || !offsets || count == 0 || count > v->max_batch) return VPBS_ERR_INVALID;
    for (size_t k = 0; k < count; ++k)
        if (offsets[k + 1] < offsets[k]) return VPBS_ERR_INVALID;
    vpbs_ctx* ctx = v->ctx;
    const Shape& S = v->S;
    const size_t total = offsets[count] - offsets[0];
    const size_t head = 8 * (count + 1);
    const size_t need = head + ((total + 7) & ~(size_t)7) + 16;
    VPBS_HIP(hipSetDevice(ctx->device));
    if (v->h_stage_bytes < need) {
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
        if (v->h_stage) (void)hipHostFree(v->h_stage);
        v->h_stage = nullptr;
        v->h_stage_bytes = 0;
        VPBS_HIP(hipHostMalloc((void**)&v->h_stage, need, hipHostMallocDefault));
        v->h_stage_bytes = need;
    }
    if (v->stage_bytes < need) {
        if (v->d_stage) ctx->release(v->d_stage);
        v->d_stage = nullptr;
        v->stage_bytes = 0;
        v->d_stage = static_cast<u64*>(ctx->alloc_bytes(need));
        v->stage_bytes = need;
    }
    u64* h_offs = reinterpret_cast<u64*>(v->h_stage);
    for (size_t k = 0; k <= count; ++k) h_offs[k] = offsets[k] - offsets[0];
    std::memcpy(v->h_stage + head, bytes + offsets[0], total);
    std::memset(v->h_stage + head + total, 0, need - head - total);
    VPBS_HIP(hipMemcpyAsync(v->d_stage, v->h_stage, need, hipMemcpyHostToDevice, ctx->stream));
    VPBS_HIP(hipMemsetAsync(v->d_flags, 0, count * sizeof(u32), ctx->stream));
    const u64* d_offs = v->d_stage;
    const u64* d_raw = v->d_stage + (count + 1);
    hipStream_t s = ctx->stream;
    const u32 n = (u32)count;
    {
        vpbs::Timed t(ctx, "vb_parse");
        const u32 span = std::max(S.n_fixed + S.max_pi, S.n_lenb);
        vb_parse<<<dim3((span + 255) / 256, n), 256, 0, s>>>(d_raw, d_offs, v->d_src, v->d_lenb_off, v->d_lenb_val, S, v->d_words, v->d_npi,
                                                             v->d_flags);
    }
    {
        vpbs::Timed t(ctx, "vb_transcript");
        vb_transcript<<<n, 16, 0, s>>>(v->d_words, v->d_npi, S, v->d_chal, v->d_flags);
    }
    if (!S.fri_only) {
        if (S.n_gates) {
            vpbs::Timed t(ctx, "vb_gates");
            vb_gates<<<dim3((n + 63) / 64, S.n_gates), 64, 0, s>>>(v->d_words, v->d_chal, v->d_gates, v->d_coset, S, n, v->d_gterms);
        }
        vpbs::Timed t(ctx, "vb_vanishing");
        vb_vanishing<<<(n + 63) / 64, 64, 0, s>>>(v->d_words, v->d_chal, v->d_gterms, S, n, v->d_flags);
    }
    {
        vpbs::Timed t(ctx, "vb_fri");
        const u64 lanes = (u64)n * S.nq;
        vb_fri<<<(unsigned)((lanes + 63) / 64), 64, 0, s>>>(v->d_words, v->d_chal, S, n, v->d_flags);
    }
    {
        vpbs::Timed t(ctx, "vb_merkle");
        const u64 lanes = (u64)n * S.nq * (4 + S.n_rounds);
        vb_merkle<<<(unsigned)((lanes + 63) / 64), 64, 0, s>>>(v->d_words, v->d_chal, v->d_cs_cap, S, n, v->d_flags);
    }
    vb_result<<<(n + 255) / 256, 256, 0, s>>>(v->d_flags, n, v->d_out);
    VPBS_HIP(hipGetLastError());
    if (view) *view = ProofBatchView{v->d_words, v->d_npi, v->d_out + count, S.W, S.n_fixed, S.max_pi};
    return VPBS_OK;
}

extern "C" {
long vpbs_proof_verifier_run(vpbs_proof_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t count, uint8_t* verdicts,
                             uint8_t* reasons) {
    if (!v || !offsets || !verdicts || count > v->max_batch) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    if (!bytes) return VPBS_ERR_INVALID;
    vpbs_ctx* ctx = v->ctx;
    try {
        const int rc = vpbs::proof_verifier_enqueue(v, bytes, offsets, count, nullptr);
        if (rc) return rc;
        // the verdicts come back through the front of the staging buffer (its offsets have been uploaded by now: same stream)
        VPBS_HIP(hipMemcpyAsync(v->h_stage, v->d_out, 2 * count, hipMemcpyDeviceToHost, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        return VPBS_ERR_DEVICE;
    }
    long accepted = 0;
    for (size_t k = 0; k < count; ++k) {
        verdicts[k] = v->h_stage[k];
        accepted += v->h_stage[k];
        if (reasons) reasons[k] = v->h_stage[count + k];
    }
    return accepted;
}
}  // extern "C"

// test_entries.h: the byte tables of a shape, on the host
extern "C" long vpbs_test_proof_byte_tables(const vpbs_verify_inputs* in, size_t src_capacity, size_t lenb_capacity, uint32_t* src, uint32_t* lenb_off,
                                            uint8_t* lenb_val, size_t* n_src, size_t* n_lenb) {
    vpbs::ProofShape S;
    ByteTables tab;
    if (!in || !src || !lenb_off || !lenb_val || !n_src || !n_lenb || !vpbs::make_proof_shape(*in, vpbs::compat_of(*in), vpbs::SHAPE_PARSE, S) ||
        tab.record(S))
        return VPBS_ERR_INVALID;
    *n_src = tab.src.size();
    *n_lenb = tab.lenb_off.size();
    if (tab.src.size() > src_capacity || tab.lenb_off.size() > lenb_capacity) return VPBS_ERR_INVALID;
    std::memcpy(src, tab.src.data(), 4 * tab.src.size());
    std::memcpy(lenb_off, tab.lenb_off.data(), 4 * tab.lenb_off.size());
    std::memcpy(lenb_val, tab.lenb_val.data(), tab.lenb_val.size());
    return (long)tab.pos;
}

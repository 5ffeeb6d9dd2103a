// Aggregation of the vPBS proofs of a batch into ONE proof (include/vpbs_prover.h).
//   statement  : leaf i = hash_no_pad of the public inputs its vPBS proof must carry; a binary tree of hash_no_pad(left || right) over the
//                leaves, padded to 2^d with the last leaf (vpbs_aggregate_root on the host; ag_leaf_pair + ag_fold_many on the device)
//   prover     : vpbs_aggregator -- the level circuits A_1 .. A_levels arrive as data; every leaf is verified before anything is proven;
//                then level by level witness plan (host) -> upload -> vpbs_prove_step, the next node's witness on a second thread.
//                vpbs_aggregator_run is vpbs_aggregator_run_many with one tree: one run body, one proof per node in prove_node
//   verifiers  : vpbs_verify_aggregate (host) and vpbs_aggregate_verifier (device): parse at level d's shape, the vk list, the proof, the root
//   device statement : ONE, for many trees in one run: ag_leaf_pair over all leaves (the LWE chain and the public-input
//                sponge of a leaf side by side in one wave), ag_fold_many per level over the trees that have it, per depth ONE batch of root
//                proofs and ag_result_many, one lane per aggregate.  vpbs_aggregate_verifier_run / _root are _run_many / _roots_many with
//                one tree, behind their own refusals
//   device witness : vpbs_aggregator_set_device_witness -- the distinct nodes of a level (of ALL trees of a run_many) in
//                chunks: child proofs uploaded once each, ag_presets_kernel, the level's full plan on a vpbs_witness_device, per node gather + proof
// The prover part is host code against the library's own C ABI, as ivc.hip is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <iterator>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gl.h"
#include "poseidon.h"
#include "context.h"
#include "verify_batch.h"
#include "program_internal.h"
#include "ivc_resident.h"
#include "test_entries.h"

namespace {
using vpbs::DeviceError;
using vpbs::report;
using u32 = uint32_t;
using u64 = uint64_t;

constexpr size_t VK = 68;                 // verifier data: circuit digest [4], constants / sigmas cap [16][4]
constexpr unsigned MAX_LEVELS = 20;
constexpr unsigned HOST_THREADS = 16;     // the most host threads a call here uses

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

unsigned depth_of(size_t count) {   // max(1, ceil(log2 count))
    unsigned d = 1;
    while (((size_t)1 << d) < count) ++d;
    return d;
}

// work(t, threads) for every t < threads = min(HOST_THREADS, the hardware's, most), each on a host thread of its own: worker t takes the
// items t, t + threads, ..
template <class Work>
void strided(size_t most, Work work) {
    const unsigned hw = std::max(1u, std::min(HOST_THREADS, std::thread::hardware_concurrency()));
    const unsigned threads = (unsigned)std::min<size_t>(hw, most);
    if (threads <= 1) return work(0u, 1u);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back(work, t, threads);
    for (auto& t : pool) t.join();
}

// ================= which nodes a level has (host only) =================
// The one statement of the padding rule (vpbs_aggregate_level_jobs in the header).  A tree of `count` leaves and depth d has m_0 = count
// entries at level 0; the 2^(d - l + 1) positions of level l - 1 stand on entry min(position, m_{l-1} - 1), so node k of level l has the
// children (min(2 k, m - 1), min(2 k + 1, m - 1)), and a node whose children are those of its left neighbour is that neighbour:
// m_l = min(2^(d - l), m_{l-1} div 2 + 1).
size_t distinct_nodes(size_t count, unsigned d, unsigned level) {
    size_t m = count;
    for (unsigned l = 1; l <= level; ++l) m = std::min((size_t)1 << (d - l), m / 2 + 1);
    return m;
}

// the distinct nodes of `level` over all trees, children as indices into the list of level - 1 -> their number (the first `capacity` written)
size_t level_jobs(const size_t* counts, size_t n_trees, unsigned level, u32* tree, u32* left, u32* right, size_t capacity) {
    size_t below = 0, n = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        const unsigned d = depth_of(counts[t]);
        if (level - 1 > d) continue;   // the tree ended below level - 1
        const size_t m = distinct_nodes(counts[t], d, level - 1);
        const size_t mine = level <= d ? distinct_nodes(counts[t], d, level) : 0;
        for (size_t k = 0; k < mine; ++k, ++n)
            if (n < capacity) {
                tree[n] = (u32)t;
                left[n] = (u32)(below + std::min(2 * k, m - 1));
                right[n] = (u32)(below + std::min(2 * k + 1, m - 1));
            }
        below += m;
    }
    return n;
}

// ================= the statement on the host =================
struct Statement {
    unsigned N, K, n_lwe;
    const u64* vk0;
    size_t count;
    const u64* testvs;
    size_t n_testv;
    const u32* testv_of;
    const u64* cts;
    const u64* out_cts;
    const u64* key_hashes;
    size_t n_keys;
    const u32* key_of;
    size_t kn() const { return (size_t)K * N; }
    size_t n_pi() const { return 2 * kn() + 9 + VK; }
    size_t tv(size_t i) const { return testv_of ? testv_of[i] : (n_testv == 1 ? 0 : i); }
    size_t key(size_t i) const { return key_of ? key_of[i] : 0; }
};

// what every entry point refuses of a statement, before it reads a word of it
bool statement_ok(const Statement& s, const char* who, std::string* msg) {
    auto no = [&](const std::string& m) {
        *msg = std::string(who) + ": " + m;
        return false;
    };
    if (s.count == 0) return no("count is 0: there is nothing to aggregate");
    if (s.N == 0 || s.K == 0 || s.kn() > (1u << 20) || s.n_lwe > (1u << 24)) return no("N, K or n_lwe out of range");
    if (!s.vk0 || !s.testvs || !s.cts || !s.out_cts || !s.key_hashes) return no("null vk0, testvs, cts, out_cts or key_hashes");
    if (s.n_testv == 0 || s.n_keys == 0) return no("no test vector or no key hash");
    if (!s.testv_of && s.n_testv != s.count && s.n_testv != 1)
        return no("testv_of is null and n_testv " + std::to_string(s.n_testv) + " is neither count " + std::to_string(s.count) + " nor 1");
    for (size_t i = 0; i < s.count; ++i) {
        if (s.testv_of && s.testv_of[i] >= s.n_testv)
            return no("testv_of[" + std::to_string(i) + "] = " + std::to_string(s.testv_of[i]) + " is not below n_testv " + std::to_string(s.n_testv));
        if (s.key_of && s.key_of[i] >= s.n_keys)
            return no("key_of[" + std::to_string(i) + "] = " + std::to_string(s.key_of[i]) + " is not below n_keys " + std::to_string(s.n_keys));
    }
    return true;
}

// s_i on the host: the public inputs laid out once per leaf, then the sponge.  false: a raw word at or above p (no proof has that statement)
bool leaf_statement_host(const Statement& s, size_t i, std::vector<u64>& pis, u64 out[4]) {
    const size_t kn = s.kn(), N = s.N;
    pis.assign(s.n_pi(), 0);
    std::memcpy(pis.data() + kn - N, s.testvs + s.tv(i) * N, 8 * N);
    pis[kn] = (u64)s.n_lwe + 2;
    std::memcpy(pis.data() + kn + 1, s.out_cts + i * kn, 8 * kn);
    std::memcpy(pis.data() + 2 * kn + 1, s.key_hashes + 4 * s.key(i), 32);
    const u64* ct = s.cts + i * ((size_t)s.n_lwe + 1);
    std::vector<u64> masks((size_t)s.n_lwe + 2, 0);   // [ct[n], ct[0] .. ct[n-1], 0]: vpbs_verify_pbs's LWE chain
    masks[0] = ct[s.n_lwe];
    for (unsigned k = 0; k < s.n_lwe; ++k) masks[k + 1] = ct[k];
    vpbs_hash_chain(masks.data(), masks.size(), 1, nullptr, pis.data() + 2 * kn + 5);
    std::memcpy(pis.data() + 2 * kn + 9, s.vk0, 8 * VK);
    for (size_t j = 0; j < pis.size(); ++j)
        if (pis[j] >= gl::P) return false;
    poseidon::hash_no_pad_host(pis.data(), pis.size(), out);
    return true;
}

// the root over the leaves; false: some raw word is at or above p
bool root_host(const Statement& s, u64 out[4]) {
    const size_t count = s.count;
    const unsigned d = depth_of(count);
    std::vector<u64> level(4 * ((size_t)1 << d));
    std::vector<uint8_t> ok(count, 1);
    strided((count + 3) / 4, [&](unsigned t, unsigned threads) {
        std::vector<u64> pis;
        for (size_t i = t; i < count; i += threads) ok[i] = leaf_statement_host(s, i, pis, level.data() + 4 * i) ? 1 : 0;
    });
    for (size_t i = 0; i < count; ++i)
        if (!ok[i]) return false;
    for (size_t i = count; i < ((size_t)1 << d); ++i) std::memcpy(level.data() + 4 * i, level.data() + 4 * (count - 1), 32);   // the padding
    for (size_t n = (size_t)1 << d; n > 1; n /= 2)
        for (size_t k = 0; k < n / 2; ++k) {
            u64 h[4];
            poseidon::hash_no_pad_host(level.data() + 8 * k, 8, h);
            std::memcpy(level.data() + 4 * k, h, 32);
        }
    std::memcpy(out, level.data(), 32);
    return true;
}

bool shape_ok(const vpbs_aggregate_shape* sh) {
    return sh && sh->level_shapes && sh->vks && sh->levels >= 1 && sh->levels <= MAX_LEVELS;
}

// A_l's verify inputs: the caller's shape with cap and digest taken from vks[l]
vpbs_verify_inputs level_inputs(const vpbs_aggregate_shape& sh, unsigned l) {
    vpbs_verify_inputs v = sh.level_shapes[l - 1];
    const u64* vk = sh.vks + VK * l;
    std::memcpy(v.circuit_digest, vk, 32);
    v.constants_sigmas_cap = vk + 4;
    v.public_inputs = nullptr;
    v.n_public_inputs = 0;
    v.fri_only = 0;
    return v;
}

size_t openings_words(const vpbs_verify_inputs& c) {
    return 2 * ((size_t)c.n_constants_sigmas + c.n_wires + c.n_zs_partial_products + c.n_quotient + c.num_challenges);
}

// ================= the statement on the device: the trees of a run, one or many =================
struct AggShape {
    u32 N, kn, n_lwe, n_pi;
};

// Leaf statements: one leaf per wave of two 16-lane groups, each with its own 48-word LDS window.  In a group lane l < 12 owns sponge
// element l (the permute_wide layout of vp_lwe_chain) and lanes 12 .. 15 only take part in the permutation.
//   Group A (lanes 0 .. 15) walks the leaf's LWE chain exactly as vp_lwe_chain: n_lwe + 2 links over [ct[n], ct[0] .. ct[n-1], 0], a link
//     puts the reduced item in element 4, zero in elements 5 .. 11 and permutes.
//   Group B (lanes 16 .. 31) is the sponge over the leaf's n_pi = 2 K N + 77 public inputs, generated here from the statement's parts (the
//     vector is never materialised).  The sponge is in overwrite mode: block b replaces the rate lanes l < 8 by public inputs 8 b + l; n_pi
//     is no multiple of 8, so the last block is partial and its upper rate lanes keep the old state.  B absorbs first the F = (2 K N + 5)
//     div 8 blocks that hold no LWE-hash word.
// Both groups call permute_wide in the same iterations -- every lane of the wave must -- and a group with nothing left permutes a value it
// discards.  After max(n_lwe + 2, F) iterations A leaves its four words in LDS behind a wavefront fence (the LDS operations of a wave execute
// in order) and B absorbs the remaining blocks, at most ten.  Critical path: max(n_lwe + 2, F) + ceil(n_pi / 8) - F permutations, where the
// chain and the sponge one after the other would take (n_lwe + 2) + ceil(n_pi / 8).  A raw word at or above p sets the flag of the leaf's
// TREE (the leaf's own result is then meaningless: no proof has that statement).  Bounds: blockIdx.x < the leaf count; testv_of[i] <
// n_testv, key_of[i] < n_keys and tree_of[i] < n_agg are checked on the host; j - 2 kn - 9 < 68.
__global__ __launch_bounds__(32) void ag_leaf_pair(const u64* __restrict__ testvs, const u32* __restrict__ testv_of, const u64* __restrict__ out_ct,
                                                   const u64* __restrict__ key_hashes, const u32* __restrict__ key_of, const u64* __restrict__ cts,
                                                   const u64* __restrict__ vk0, const u32* __restrict__ tree_of, AggShape S, u64* __restrict__ stmt,
                                                   u32* __restrict__ flags) {
    __shared__ u64 sh[2 * poseidon::WIDE_LDS_WORDS + 4];
    const unsigned l = threadIdx.x & 15, g = threadIdx.x >> 4;
    u64* win = sh + g * poseidon::WIDE_LDS_WORDS;
    u64* hand = sh + 2 * poseidon::WIDE_LDS_WORDS;   // the end of the LWE chain, from A to B
    const u32 i = blockIdx.x;
    const u64* c = cts + (u64)i * (S.n_lwe + 1);
    const u64* tv = testvs + (u64)testv_of[i] * S.N;
    const u64* oc = out_ct + (u64)i * S.kn;
    const u64* kh = key_hashes + (u64)key_of[i] * 4;
    auto word = [&](u32 j) -> u64 {
        if (j < S.kn - S.N) return 0;
        if (j < S.kn) return tv[j - (S.kn - S.N)];
        if (j == S.kn) return (u64)S.n_lwe + 2;
        if (j <= 2 * S.kn) return oc[j - S.kn - 1];
        if (j < 2 * S.kn + 5) return kh[j - 2 * S.kn - 1];
        if (j < 2 * S.kn + 9) return hand[j - 2 * S.kn - 5];
        return vk0[j - 2 * S.kn - 9];
    };
    const u32 links = S.n_lwe + 2, F = (2 * S.kn + 5) / 8, both = max(links, F);
    const bool rate = g == 1 && l < 8;
    u64 x = 0;
    bool bad = false;
    // the next item / block is loaded while this one runs: the loads are off the dependent chain.  Words below 8 F never come from `hand`.
    u64 next = g == 0 ? c[S.n_lwe] : (rate && l < 8 * F ? word(l) : 0);
    for (u32 it = 0; it < both; ++it) {
        const u64 cur = next;
        u64 in = x;
        if (g == 0) {
            next = it < S.n_lwe ? c[it] : 0;
            if (l == 4) in = gl::canon(cur);
            else if (l > 4) in = 0;
        } else {
            const u32 jn = 8 * (it + 1) + l;
            next = rate && jn < 8 * F ? word(jn) : 0;
            if (rate && it < F) {
                bad = bad || cur >= gl::P;
                in = gl::canon(cur);
            }
        }
        const u64 y = poseidon::permute_wide(in, win, l);
        if (it < (g == 0 ? links : F)) x = y;
    }
    if (g == 0 && l < 4) hand[l] = x;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    next = rate && 8 * F + l < S.n_pi ? word(8 * F + l) : 0;
    for (u32 off = 8 * F; off < S.n_pi; off += 8) {
        const bool mine = rate && off + l < S.n_pi;
        const u64 w = next;
        const u32 jn = off + 8 + l;
        next = rate && jn < S.n_pi ? word(jn) : 0;
        u64 in = x;
        if (mine) {
            bad = bad || w >= gl::P;
            in = gl::canon(w);
        }
        const u64 y = poseidon::permute_wide(in, win, l);
        if (g == 1) x = y;
    }
    if (g == 1 && l < 4) stmt[(u64)i * 4 + l] = x;
    if (bad) atomicOr(&flags[tree_of[i]], 1u);
}

// what the segmented fold knows of one tree at one level: its entries of the level below (n_in of them from in_first: the tree's own leaf
// count at level 1, the whole level above that), where its nodes start in this level, and whether this level is the tree's depth
struct FoldTree {
    u32 in_first, n_in, out_first, root;
};

// One level of ALL trees that still have that level, one node per 16-lane block: node k of a tree = hash_no_pad(in[2k] || in[2k + 1]), one
// permutation of [left, right, 0 0 0 0]; node_tree[node] names the node's tree.  A tree's entries at or past its n_in read its entry
// n_in - 1: at the leaves (n_in = the tree's own count) that index clamp IS the padding rule, so a one-leaf tree folds its leaf with itself;
// above them n_in is the tree's whole level and nothing is clamped.  The node of a tree's own depth also lands in roots[tree].  Bounds:
// blockIdx.x < the level's node count, node_tree[..] < n_agg, in_first + n_in within the level below (the host builds the tables from the
// checked leaf counts).
__global__ __launch_bounds__(16) void ag_fold_many(const u64* __restrict__ in, const u32* __restrict__ node_tree, const FoldTree* __restrict__ tab,
                                                   u64* __restrict__ out, u64* __restrict__ roots) {
    __shared__ u64 sh[poseidon::WIDE_LDS_WORDS];
    const unsigned l = threadIdx.x;
    const u32 node = blockIdx.x, t = node_tree[node];
    const FoldTree T = tab[t];
    const u32 k = node - T.out_first;
    const u32 a = T.in_first + min(2 * k, T.n_in - 1), b = T.in_first + min(2 * k + 1, T.n_in - 1);
    u64 x = 0;
    if (l < 4) x = in[(u64)a * 4 + l];
    else if (l < 8) x = in[(u64)b * 4 + l - 4];
    x = poseidon::permute_wide(x, sh, l);
    if (l < 4) {
        out[(u64)node * 4 + l] = x;
        if (T.root) roots[(u64)t * 4 + l] = x;
    }
}

// The verdicts of the n aggregates of one depth d, one lane each: proof i of the depth's batch is aggregate a = agg_of[i].  The first failing
// check in vpbs_verify_aggregate's order -- MALFORMED (the batch verifier could not parse the bytes, or they do not carry n_expected = 4 + 68 d
// public inputs), VERIFIER_DATA (public inputs 4 .. against vks), PROOF (the batch verifier's verdict), ROOT (public inputs 0 .. 3 against
// the tree's own root, or the tree's raw-word flag) -> out[2 a] = verdict, out[2 a + 1] = reason.  The public inputs are read as the batch
// verifier parsed them: n_expected words are inside its slot whatever the bytes were (the host checks max_pi).
__global__ __launch_bounds__(64) void ag_result_many(const uint8_t* __restrict__ proof_reason, const u32* __restrict__ n_pi,
                                                     const u64* __restrict__ words, u32 W, u32 n_fixed, const u64* __restrict__ vks,
                                                     const u64* __restrict__ roots, const u32* __restrict__ flags, const u32* __restrict__ agg_of,
                                                     u32 n, u32 n_expected, uint8_t* __restrict__ out) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const u32 a = agg_of[i];
    const u64* pis = words + (u64)i * W + n_fixed;
    const u64* root = roots + (u64)a * 4;
    const uint8_t pr = proof_reason[i];
    uint8_t reason = VPBS_AGG_OK;
    if (pr == VPBS_VERIFY_MALFORMED || n_pi[i] != n_expected) {
        reason = VPBS_AGG_MALFORMED;
    } else {
        bool vk_bad = false, root_bad = flags[a] != 0;
        for (u32 j = 4; j < n_expected; ++j) vk_bad = vk_bad || pis[j] != vks[j - 4];
        for (u32 j = 0; j < 4; ++j) root_bad = root_bad || pis[j] != root[j];
        reason = vk_bad ? VPBS_AGG_VERIFIER_DATA : pr != VPBS_VERIFY_OK ? VPBS_AGG_PROOF : root_bad ? VPBS_AGG_ROOT : VPBS_AGG_OK;
    }
    out[2 * a] = reason == VPBS_AGG_OK ? 1 : 0;
    out[2 * a + 1] = reason;
}

// ================= the preset matrix of a chunk of nodes, on the device =================
// rows [n_rows][row_words]: the distinct child proofs of the chunk, each flat | pis; tab [batch][2]: the (left row, right row) of every node;
// vks: vk_0 .. vk_{l-1} as the level takes them.  The matrix is [2 row_words + vk_words][batch], instances innermost, in the order
// vpbs_aggregator_create documents: slot 0 proof | slot 0 public inputs | slot 1 proof | slot 1 public inputs | vk_0 .. vk_{l-1}.
struct PresetJob {
    const u64* rows;
    const u32* tab;
    const u64* vks;
    u32 row_words, vk_words, batch;
};

// blockIdx.z = slot 0 / 1: per node a contiguous child row, in the matrix one column.  A workgroup turns a tile of 32 nodes x 64 words in
// LDS, as preset_transpose_kernel (pbs_prove_pool.hip) does for the chains: the rows are read coalesced (64 lanes on 512 contiguous bytes),
// the columns written coalesced (32 lanes on the 32 instances of a matrix row); a tile row is padded by one word, so the 32 lanes of a half-wave
// read words 65 apart -- all 64 banks, no conflict.  blockIdx.z = 2: the vk rows, every word broadcast over its row, consecutive lanes on
// consecutive instances.  Bounds: tab[..] < n_rows (the host builds both from the same list), k0 + k < row_words and i < batch are tested.
constexpr unsigned AG_TILE_I = 32, AG_TILE_K = 64;
__global__ void __launch_bounds__(256) ag_presets_kernel(PresetJob j, u64* __restrict__ m) {
    __shared__ u64 tile[AG_TILE_I][AG_TILE_K + 1];
    if (blockIdx.z == 2) {
        const size_t words = (size_t)j.vk_words * j.batch, stride = (size_t)gridDim.x * gridDim.y * 256;
        for (size_t q = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; q < words; q += stride)
            m[2 * (size_t)j.row_words * j.batch + q] = j.vks[q / j.batch];
        return;
    }
    const u32 slot = blockIdx.z, k0 = blockIdx.x * AG_TILE_K, i0 = blockIdx.y * AG_TILE_I;
    for (unsigned ii = threadIdx.x / AG_TILE_K; ii < AG_TILE_I; ii += 256 / AG_TILE_K) {
        const unsigned k = threadIdx.x % AG_TILE_K, i = i0 + ii;
        u64 v = 0;
        if (i < j.batch && k0 + k < j.row_words) v = j.rows[(size_t)j.tab[2 * i + slot] * j.row_words + k0 + k];
        tile[ii][k] = v;
    }
    __syncthreads();
    for (unsigned k = threadIdx.x / AG_TILE_I; k < AG_TILE_K; k += 256 / AG_TILE_I) {
        const unsigned ii = threadIdx.x % AG_TILE_I;
        if (k0 + k < j.row_words && i0 + ii < j.batch) m[((size_t)slot * j.row_words + k0 + k) * j.batch + i0 + ii] = tile[ii][k];
    }
}

// the fill of vpbs::witness_device_run_filled: user is the chunk's PresetJob
int presets_fill(void* user, void* stream, uint64_t* d_matrix) {
    const PresetJob& j = *static_cast<const PresetJob*>(user);
    hipLaunchKernelGGL(ag_presets_kernel, dim3((j.row_words + AG_TILE_K - 1) / AG_TILE_K, (j.batch + AG_TILE_I - 1) / AG_TILE_I, 3), dim3(256), 0,
                       static_cast<hipStream_t>(stream), j, d_matrix);
    return hipGetLastError() == hipSuccess ? VPBS_OK : VPBS_ERR_DEVICE;
}
}  // namespace

struct vpbs_aggregate_verifier {
    vpbs_ctx* ctx = nullptr;
    unsigned N = 0, K = 0, n_lwe = 0, levels = 0;
    size_t max_leaves = 0;
    size_t max_aggregates = 1;                  // the trees of one run at most (create: 1)
    std::vector<vpbs_proof_verifier*> proofs;   // [levels]: the batch verifier of A_l's proofs, batches of max_aggregates
    std::vector<void*> owned;
    u64 *d_vks = nullptr, *d_in = nullptr, *d_stmt = nullptr;    // vk_0 .. vk_levels; h_in's image; the leaf statements [max_leaves][4]
    u64* h_in = nullptr;      // pinned: cts | out_cts | testvs | key_hashes
    // A level of all trees [max_leaves][4], twice; roots [max_aggregates][4].  A level never has more nodes than there are leaves: a tree
    // of count >= 2 leaves and depth d has 2^(d - 1) < count nodes at level 1 and fewer above, a tree of one leaf has one node.
    u64 *d_mnodes[2] = {nullptr, nullptr}, *d_roots = nullptr;
    u32 *d_mflags = nullptr, *d_midx = nullptr;                  // raw-word flag per tree; the index tables of a run (many_idx_words)
    uint8_t* d_mout = nullptr;                                   // verdict, reason per aggregate
    u32* h_midx = nullptr;    // pinned: d_midx's image
    u64* h_mout = nullptr;    // pinned: roots [max_aggregates][4] | flags or verdict, reason [max_aggregates]
    // testv_of, key_of, tree_of per leaf | node_tree of every level (a tree of count leaves has 2^d - 1 < 2 count nodes over its levels:
    // fewer than 2 max_leaves in all) | FoldTree per tree and level | agg_of per aggregate
    size_t many_idx_words() const { return 5 * max_leaves + (4 * (size_t)levels + 1) * max_aggregates + 16; }
    std::mutex mu;
    size_t kn() const { return (size_t)K * N; }
    // the leaf count, n_testv and n_keys of a run are at most max_leaves each
    size_t in_words() const { return max_leaves * ((size_t)n_lwe + 1 + kn() + N + 4); }
    void* alloc(size_t bytes) {
        void* d = ctx->alloc_bytes(std::max<size_t>(8, bytes));
        owned.push_back(d);
        return d;
    }
    ~vpbs_aggregate_verifier() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
        if (h_in) (void)hipHostFree(h_in);
        if (h_midx) (void)hipHostFree(h_midx);
        if (h_mout) (void)hipHostFree(h_mout);
        for (auto* p : proofs) vpbs_proof_verifier_free(p);
    }
};

// ================= the prover =================
namespace {
struct Level {   // one circuit A_l on the context
    vpbs_ctx* ctx = nullptr;
    unsigned log_n = 0, n_wires = 0, n_routed = 0, n_const_cols = 0, num_selectors = 0;
    size_t n = 0, n_pi = 0, n_preset = 0, inner_words = 0, inner_pi = 0;
    std::vector<vpbs_gate> gates;
    std::vector<uint32_t> pi_pos;
    std::vector<u64> vk;
    u64* d_sigma = nullptr;
    vpbs_batch* cs = nullptr;
    vpbs_witness_plan* plan = nullptr;
    vpbs_witness_device* wd = nullptr;   // the plan on the device, for batches of nodes (vpbs_aggregator_set_device_witness)
    vpbs_step_sizes sz{};
    size_t proof_words() const { return 3 * sz.cap_words + sz.openings_words + sz.fri_words; }

    void step_inputs(vpbs_step_inputs& in, const u64* d_wires, const u64* pis) const {
        in = vpbs_step_inputs{};
        in.log_n = log_n; in.n_wires = n_wires; in.n_zs_partial_products = 20; in.n_quotient = 16; in.num_challenges = 2;
        in.inputs_on_device = 1;
        in.wires_values = d_wires;
        in.constants_sigmas = cs;
        for (int i = 0; i < 4; ++i) in.circuit_digest[i] = vk[i];
        in.public_inputs = pis; in.n_public_inputs = n_pi;
        in.forced_pow = VPBS_POW_ANY;
        in.sigmas_values = d_sigma; in.sigmas_on_device = 1;
        in.n_routed = n_routed; in.quotient_degree_factor = 8; in.n_constants = n_const_cols;
        in.gates = gates.data(); in.n_gates = (unsigned)gates.size(); in.num_selectors = num_selectors;
    }
    int init(vpbs_ctx* c, const vpbs_ivc_circuit& d, std::string& err) {
        ctx = c;
        const vpbs_circuit& k = *d.circuit;
        log_n = k.log_n; n_wires = k.n_wires; n_routed = k.n_routed; n_const_cols = k.n_constants_cols; num_selectors = k.num_selectors;
        n = (size_t)1 << log_n;
        gates.assign(k.gates, k.gates + k.n_gates);
        pi_pos.assign(d.pi_pos, d.pi_pos + d.n_pi);
        n_pi = d.n_pi;
        n_preset = d.n_preset;
        inner_words = d.proof_words;
        std::vector<u64> csv((size_t)(n_const_cols + n_routed) * n);
        std::memcpy(csv.data(), k.constants, 8 * (size_t)n_const_cols * n);
        u64* sigma = csv.data() + (size_t)n_const_cols * n;
        if (vpbs_sigma_values(&k, sigma) != 0) return err = "sigma polynomials: malformed copy constraints", VPBS_ERR_INVALID;
        std::vector<u64> cap(VK - 4);
        int rc = vpbs_commit_values(ctx, csv.data(), n_const_cols + n_routed, log_n, &cs, cap.data());
        if (rc != 0) return err = std::string("constants / sigmas commitment: ") + vpbs_last_error(ctx), rc;
        vk.assign(4, 0);
        vpbs_compat compat;
        vpbs_ctx_get_compat(ctx, &compat);
        vpbs_circuit_digest(&compat, cap.data(), cap.size(), log_n, vk.data());
        vk.insert(vk.end(), cap.begin(), cap.end());
        rc = vpbs_device_alloc(ctx, (size_t)n_routed * n, &d_sigma);
        if (rc == 0) rc = vpbs_device_upload(ctx, d_sigma, sigma, (size_t)n_routed * n);
        if (rc != 0) return err = std::string("sigma values to the device: ") + vpbs_last_error(ctx), rc;
        char e[256] = {0};
        rc = vpbs_witness_plan_create(&k, d.preset_pos, d.n_preset, &plan, e, sizeof e);
        if (rc != 0) return err = std::string("witness plan: ") + e, rc;
        vpbs_step_inputs in;
        step_inputs(in, nullptr, nullptr);
        if (vpbs_step_sizes_get(ctx, &in, &sz) != 0) return err = "no step proof of this shape", VPBS_ERR_INVALID;
        return VPBS_OK;
    }
    void release() {
        if (wd) vpbs_witness_device_free(wd);   // before the plan it replays
        wd = nullptr;
        if (plan) vpbs_witness_plan_free(plan);
        if (cs) vpbs_batch_free(cs);
        if (d_sigma) vpbs_device_free(ctx, d_sigma);
        plan = nullptr; cs = nullptr; d_sigma = nullptr;
    }
};

struct Proof {   // a leaf or a node: the flat proof words (caps, openings, FRI) and the public inputs
    std::vector<u64> flat, pis;
};
}  // namespace

struct vpbs_aggregator {
    vpbs_ctx* ctx = nullptr;
    vpbs_verify_inputs leaf{};
    std::vector<vpbs_gate> leaf_gates;
    std::vector<u64> vk0;
    size_t leaf_n_pi = 0, leaf_words = 0;
    std::vector<Level> levels;
    u64 *bufs[2] = {nullptr, nullptr}, *d_wires = nullptr;
    size_t wire_words = 0;
    vpbs_aggregate_stats last{};
    // the device witness: at most max_nodes nodes per batch (0: the host path); the child rows of a chunk and behind them its
    // (left row, right row) table, pinned and on the device; vk_0 .. vk_{levels-1} resident; the last run's figures
    unsigned max_nodes = 0;
    size_t row_words_max = 0;
    u64 *h_rows = nullptr, *d_rows = nullptr, *d_vks = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    uint64_t dev_stats[4] = {0, 0, 0, 0};
    std::mutex mu;
    void device_witness_off() {
        for (auto& l : levels)
            if (l.wd) {
                vpbs_witness_device_free(l.wd);
                l.wd = nullptr;
            }
        if (h_rows) (void)hipHostFree(h_rows);
        if (d_rows) vpbs_device_free(ctx, d_rows);
        if (d_vks) vpbs_device_free(ctx, d_vks);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        h_rows = d_rows = d_vks = nullptr;
        ev[0] = ev[1] = nullptr;
        max_nodes = 0;
    }
    ~vpbs_aggregator() {
        device_witness_off();
        for (auto b : bufs)
            if (b) vpbs_host_free(b);
        if (d_wires) vpbs_device_free(ctx, d_wires);
        for (auto& l : levels) l.release();
    }
};

namespace {
// ---- every leaf is parsed, verified and compared with vk_0 before anything is proven: cur[i] the leaf, why[i] "" or what is wrong with it ----
void check_leaves(const vpbs_aggregator* a, const uint8_t* bytes, const size_t* offsets, size_t count, std::vector<Proof>& cur,
                  std::vector<std::string>& why) {
    cur.assign(count, Proof{});
    why.assign(count, "");
    const size_t cap3 = 3 * ((size_t)4 << 4), op = openings_words(a->leaf), fri_words = a->leaf_words - cap3 - op;
    strided(count, [&](unsigned t, unsigned threads) {
        for (size_t i = t; i < count; i += threads) {
            Proof& p = cur[i];
            const size_t len = offsets[i + 1] - offsets[i];
            p.pis.assign(a->leaf_n_pi, 0);
            std::vector<u64> fri(std::max(fri_words, len / 8 + 8));
            p.flat.assign(a->leaf_words, 0);
            const long n = vpbs_step_proof_from_bytes(&a->leaf, bytes + offsets[i], len, p.flat.data(), p.flat.data() + cap3, fri.data(), p.pis.data(),
                                                      a->leaf_n_pi);
            // a proof of the leaf shape has exactly leaf_words words: the parser accepts no other length of FRI section
            if (n != (long)a->leaf_n_pi || 8 * (a->leaf_words + a->leaf_n_pi) > len) {
                why[i] = "the bytes are not a vPBS proof of the leaf circuit (shape, canonical field elements, number of public inputs)";
                continue;
            }
            std::memcpy(p.flat.data() + cap3 + op, fri.data(), 8 * fri_words);
            if (std::memcmp(p.pis.data() + a->leaf_n_pi - VK, a->vk0.data(), 8 * VK) != 0) {
                why[i] = "the proof carries other verifier data than vk_0";
                continue;
            }
            vpbs_verify_inputs v = a->leaf;
            v.public_inputs = p.pis.data();
            v.n_public_inputs = a->leaf_n_pi;
            if (vpbs_verify_step(&v, p.flat.data(), p.flat.data() + cap3, fri.data()) != 1) why[i] = "the proof does not verify";
        }
    });
}

// a root node's proof, serialised -> the number of bytes, or < 0 with msg
long root_bytes(vpbs_aggregator* a, const Level& L, const Proof& p, uint8_t* out, size_t capacity, std::string& msg) {
    vpbs_step_inputs in{};
    L.step_inputs(in, a->d_wires, p.pis.data());
    const u64 *cp = p.flat.data(), *opn = cp + 3 * L.sz.cap_words, *fr = opn + L.sz.openings_words;
    const long n = vpbs_step_proof_to_bytes(a->ctx, &in, L.n_const_cols, cp, opn, fr, out, capacity);
    if (n > 0) return n;
    msg = "the output buffer is too small for the aggregate proof";
    return VPBS_ERR_INVALID;
}

// One node's proof, on either path: its wires are in a->d_wires and p.pis is filled -> p.flat.  The time goes to last.prove_ms; a proven
// node is counted.  VPBS_OK, or the prover's status with msg.
int prove_node(vpbs_aggregator* a, const Level& L, Proof& p, std::string& msg) {
    const double t0 = now();
    vpbs_step_inputs in{};
    p.flat.assign(L.proof_words(), 0);
    L.step_inputs(in, a->d_wires, p.pis.data());
    u64 *cp = p.flat.data(), *opn = cp + 3 * L.sz.cap_words, *fr = opn + L.sz.openings_words;
    const int rc = vpbs_prove_step(a->ctx, &in, cp, opn, fr, nullptr, nullptr);
    a->last.prove_ms += 1e3 * (now() - t0);
    if (rc != 0) return msg = std::string("proof: ") + vpbs_last_error(a->ctx), rc;
    ++a->last.nodes;
    return VPBS_OK;
}

// where a tree's root goes once the level of its depth is through: the number of bytes it serialised, or < 0 (with the run's msg set), which ends the run
using RootFn = std::function<long(size_t tree, const Level& L, const Proof& p)>;

// ---- tree `t` on the host path, level by level: its checked leaves in `cur` -> its root to `root`; what that returns, or < 0 with msg ----
long tree_host(vpbs_aggregator* a, std::vector<Proof>& cur, size_t count, size_t t, const RootFn& root, std::string& msg) {
    const unsigned d = depth_of(count);
    std::vector<u64> vks((a->levels.size() + 1) * VK);
    vpbs_aggregator_verifier_data(a, vks.data());
    for (unsigned l = 1; l <= d; ++l) {
        const Level& L = a->levels[l - 1];
        // the distinct nodes of this level, in order, and which proofs of `cur` they stand on
        std::vector<u32> tree(level_jobs(&count, 1, l, nullptr, nullptr, nullptr, 0)), left(tree.size()), right(tree.size());
        level_jobs(&count, 1, l, tree.data(), left.data(), right.data(), tree.size());
        std::vector<Proof> next(tree.size());
        std::string werr[2];
        double wms[2] = {0, 0};
        auto witness = [&](size_t j) {   // the node's PartialWitness in the circuit's order, then the plan
            const double t0 = now();
            const Proof &x = cur[left[j]], &y = cur[right[j]];
            std::vector<u64> vals;
            vals.reserve(L.n_preset);
            vals.insert(vals.end(), x.flat.begin(), x.flat.end());
            vals.insert(vals.end(), x.pis.begin(), x.pis.end());
            vals.insert(vals.end(), y.flat.begin(), y.flat.end());
            vals.insert(vals.end(), y.pis.begin(), y.pis.end());
            vals.insert(vals.end(), vks.begin(), vks.begin() + VK * l);
            char e[256] = {0};
            werr[j & 1].clear();
            if (vals.size() != L.n_preset) werr[j & 1] = "the children do not have the circuit's shape";
            else if (vpbs_witness_plan_run(L.plan, vals.data(), 8, a->bufs[j & 1], e, sizeof e) != 0) werr[j & 1] = std::string("witness: ") + e;
            wms[j & 1] = 1e3 * (now() - t0);
        };
        witness(0);
        for (size_t j = 0; j < next.size(); ++j) {
            const std::string at = "level " + std::to_string(l) + ", node " + std::to_string(j) + ": ";
            a->last.witness_ms += wms[j & 1];
            if (!werr[j & 1].empty()) return msg = at + werr[j & 1], VPBS_ERR_INVALID;
            const u64* wires = a->bufs[j & 1];
            Proof& p = next[j];
            p.pis.resize(L.n_pi);
            for (size_t i = 0; i < L.n_pi; ++i) p.pis[i] = wires[L.pi_pos[i]];
            std::string why;
            int rc = vpbs_device_upload(a->ctx, a->d_wires, wires, (size_t)L.n_wires * L.n);
            if (rc != 0) why = std::string("proof: ") + vpbs_last_error(a->ctx);
            std::thread ahead;   // the next node's witness while this one is being proven (the other buffer)
            if (j + 1 < next.size()) ahead = std::thread(witness, j + 1);
            if (rc == 0) rc = prove_node(a, L, p, why);
            if (ahead.joinable()) ahead.join();
            if (rc != 0) return msg = at + why, (long)rc;
        }
        cur.swap(next);
    }
    return root(t, a->levels[d - 1], cur[0]);
}

// the child rows of a chunk and its (left row, right row) table, staged in h_rows and queued for d_rows on the context's stream -> the job
// ag_presets_kernel takes.  ids: the DISTINCT children of the chunk, ascending; pairs [batch][2]: every node's children, as entries of ids.
PresetJob presets_upload(vpbs_aggregator* a, const Level& L, unsigned l, const std::vector<const Proof*>& rows, const u32* pairs, unsigned batch) {
    const size_t row_words = L.inner_words + L.inner_pi;
    for (size_t r = 0; r < rows.size(); ++r) {
        std::memcpy(a->h_rows + r * row_words, rows[r]->flat.data(), 8 * L.inner_words);
        std::memcpy(a->h_rows + r * row_words + L.inner_words, rows[r]->pis.data(), 8 * L.inner_pi);
    }
    std::memcpy(a->h_rows + rows.size() * row_words, pairs, 8 * (size_t)batch);
    VPBS_HIP(hipMemcpyAsync(a->d_rows, a->h_rows, 8 * (rows.size() * row_words + batch), hipMemcpyHostToDevice, a->ctx->stream));
    return PresetJob{a->d_rows, reinterpret_cast<const u32*>(a->d_rows + rows.size() * row_words), a->d_vks, (u32)row_words, (u32)(VK * l), batch};
}

// ---- the trees of a run on the device path, level by level over ALL of them: the checked leaves of all trees in `cur`, concatenated.  A tree's
// root goes to `root` after the level of its depth.  VPBS_OK, or < 0 with msg ----
long trees_device(vpbs_aggregator* a, std::vector<Proof>& cur, const size_t* counts, size_t n_trees, const RootFn& root, std::string& msg) {
    vpbs_ctx* ctx = a->ctx;
    unsigned deepest = 0;
    for (size_t t = 0; t < n_trees; ++t) deepest = std::max(deepest, depth_of(counts[t]));
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        for (unsigned l = 1; l <= deepest; ++l) {
            const Level& L = a->levels[l - 1];
            const std::string at = "level " + std::to_string(l) + ": ";
            std::vector<u32> tree(level_jobs(counts, n_trees, l, nullptr, nullptr, nullptr, 0)), left(tree.size()), right(tree.size());
            level_jobs(counts, n_trees, l, tree.data(), left.data(), right.data(), tree.size());
            std::vector<Proof> next(tree.size());
            for (size_t first = 0; first < tree.size(); first += a->max_nodes) {
                const unsigned batch = (unsigned)std::min<size_t>(a->max_nodes, tree.size() - first);
                // 1. every distinct child of the chunk once; 2. + 3. the preset matrix and the plan behind the upload, on the context's stream
                const double t0 = now();
                std::vector<u32> ids;
                for (unsigned j = 0; j < batch; ++j) {
                    ids.push_back(left[first + j]);
                    ids.push_back(right[first + j]);
                }
                std::sort(ids.begin(), ids.end());
                ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
                std::vector<const Proof*> rows;
                for (u32 id : ids) {
                    if (cur[id].flat.size() != L.inner_words || cur[id].pis.size() != L.inner_pi) return msg = at + "the children do not have the circuit's shape", VPBS_ERR_INVALID;
                    rows.push_back(&cur[id]);
                }
                std::vector<u32> pairs(2 * (size_t)batch);
                for (unsigned j = 0; j < batch; ++j) {
                    pairs[2 * j] = (u32)(std::lower_bound(ids.begin(), ids.end(), left[first + j]) - ids.begin());
                    pairs[2 * j + 1] = (u32)(std::lower_bound(ids.begin(), ids.end(), right[first + j]) - ids.begin());
                }
                VPBS_HIP(hipEventRecord(a->ev[0], ctx->stream));
                PresetJob job = presets_upload(a, L, l, rows, pairs.data(), batch);
                const int wrc = vpbs::witness_device_run_filled(L.wd, batch, presets_fill, &job);
                const std::string werr = wrc != 0 ? vpbs_last_error(ctx) : "";
                VPBS_HIP(hipEventRecord(a->ev[1], ctx->stream));
                VPBS_HIP(hipEventSynchronize(a->ev[1]));
                float ms = 0;
                VPBS_HIP(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
                a->last.witness_ms += 1e3 * (now() - t0);
                ++a->dev_stats[1];
                a->dev_stats[2] += (uint64_t)(1e3 * ms);
                if (wrc != 0) return msg = at + "witness: " + werr, (long)wrc;
                // 4. node by node: the public inputs, the wires into the device matrix, the proof
                for (unsigned j = 0; j < batch; ++j) {
                    const size_t node = first + j;
                    const std::string at_node = "level " + std::to_string(l) + ", node " + std::to_string(node) + ": ";
                    Proof& p = next[node];
                    p.pis.resize(L.n_pi);
                    const double tg = now();
                    int rc = vpbs_witness_device_read(L.wd, j, L.pi_pos.data(), L.n_pi, p.pis.data());
                    if (rc == 0) rc = vpbs_witness_device_wires(L.wd, j, a->d_wires);
                    a->dev_stats[3] += (uint64_t)(1e6 * (now() - tg));
                    if (rc != 0) return msg = at_node + "gather: " + vpbs_last_error(ctx), (long)rc;
                    std::string why;
                    rc = prove_node(a, L, p, why);
                    if (rc != 0) return msg = at_node + why, (long)rc;
                    ++a->dev_stats[0];
                }
            }
            // a tree whose depth this level is has exactly one node here: its root
            for (size_t node = 0; node < tree.size(); ++node)
                if (depth_of(counts[tree[node]]) == l) {
                    const long rc = root(tree[node], L, next[node]);
                    if (rc < 0) return rc;
                }
            cur.swap(next);
        }
    } catch (const DeviceError& e) {
        (void)vpbs::stream_sync(ctx->stream);
        ctx->err = e.what;
        msg = e.what;
        return e.status;
    }
    return VPBS_OK;
}

// a run starts from zeroed figures, whatever it goes on to refuse
void reset_stats(vpbs_aggregator* a) {
    a->last = vpbs_aggregate_stats{};
    std::memset(a->dev_stats, 0, sizeof a->dev_stats);
}

// ---- The body of vpbs_aggregator_run (one tree) and _run_many, under the aggregator's lock, after reset_stats and the wrapper's own
// refusals (1 <= counts[t] <= 2^levels, fewer than 2^32 leaves, no null pointer).  `many`: trees are named -- a bad leaf is "tree t, leaf
// i", not "leaf i", and what fails in tree t on the host path starts "tree t: ".  root takes the roots.  VPBS_OK, or < 0 with msg ----
long run_body(vpbs_aggregator* a, const uint8_t* bytes, const size_t* offsets, const size_t* counts, size_t n_trees, bool many, const RootFn& root,
              std::string& msg) {
    const auto tree = [](size_t t) { return "tree " + std::to_string(t); };
    std::vector<size_t> first(n_trees + 1, 0);
    for (size_t t = 0; t < n_trees; ++t) first[t + 1] = first[t] + counts[t];
    const size_t total = first[n_trees];
    for (size_t i = 0; i < total; ++i)
        if (offsets[i + 1] < offsets[i]) return msg = "offsets decrease at leaf " + std::to_string(i), VPBS_ERR_INVALID;
    const double t_start = now();
    for (size_t t = 0; t < n_trees; ++t) a->last.depth = std::max(a->last.depth, depth_of(counts[t]));
    // ---- ALL leaves of all trees before anything is proven ----
    std::vector<Proof> cur;
    std::vector<std::string> why;
    check_leaves(a, bytes, offsets, total, cur, why);
    a->last.check_leaves_ms = 1e3 * (now() - t_start);
    long rc = VPBS_OK;
    for (size_t t = 0; t < n_trees && rc == VPBS_OK; ++t)
        for (size_t i = first[t]; i < first[t + 1] && rc == VPBS_OK; ++i)
            if (!why[i].empty()) {
                msg = (many ? tree(t) + ", leaf " : "leaf ") + std::to_string(i - first[t]) + ": " + why[i] + "; nothing was proven";
                rc = VPBS_ERR_INVALID;
            }
    if (rc == VPBS_OK && a->max_nodes) {   // the device witness: the levels of all trees in chunks
        rc = trees_device(a, cur, counts, n_trees, root, msg);
    } else if (rc == VPBS_OK) {            // the host path: the trees one after the other
        for (size_t t = 0; t < n_trees && rc >= 0; ++t) {
            std::vector<Proof> leaves(std::make_move_iterator(cur.begin() + first[t]), std::make_move_iterator(cur.begin() + first[t + 1]));
            rc = tree_host(a, leaves, counts[t], t, root, msg);
            if (rc < 0 && many) msg = tree(t) + ": " + msg;
        }
    }
    a->last.seconds = now() - t_start;
    return rc < 0 ? rc : VPBS_OK;
}
}  // namespace

extern "C" {

const char* vpbs_aggregate_reason_text(int reason) {
    switch (reason) {
        case VPBS_AGG_OK: return "";
        case VPBS_AGG_MALFORMED: return "the bytes are not an aggregate proof of this depth (shape, canonical field elements, number of public inputs)";
        case VPBS_AGG_VERIFIER_DATA: return "the aggregate carries other verifier data than the expected circuits'";
        case VPBS_AGG_PROOF: return "the aggregate proof does not verify";
        case VPBS_AGG_ROOT: return "the aggregate's root is not the root of this statement";
        default: return nullptr;
    }
}

int vpbs_aggregate_root(unsigned N, unsigned K, unsigned n_lwe, const uint64_t* vk0, size_t count, const uint64_t* testvs, size_t n_testv,
                        const uint32_t* testv_of, const uint64_t* cts, const uint64_t* out_cts, const uint64_t* key_hashes, size_t n_keys,
                        const uint32_t* key_of, uint64_t out[4]) {
    const Statement s{N, K, n_lwe, vk0, count, testvs, n_testv, testv_of, cts, out_cts, key_hashes, n_keys, key_of};
    std::string msg;
    if (!out || !statement_ok(s, "vpbs_aggregate_root", &msg)) return VPBS_ERR_INVALID;
    u64 root[4];
    if (!root_host(s, root)) return 1;
    std::memcpy(out, root, 32);
    return VPBS_OK;
}

int vpbs_verify_aggregate(const vpbs_aggregate_shape* shape, size_t count, const uint64_t* testvs, size_t n_testv, const uint32_t* testv_of,
                          const uint64_t* cts, const uint64_t* out_cts, const uint64_t* key_hashes, size_t n_keys, const uint32_t* key_of,
                          const uint8_t* bytes, size_t len, int* reason, char* why, size_t why_len) {
    auto verdict = [&](int r) {
        if (reason) *reason = r;
        report(why, why_len, vpbs_aggregate_reason_text(r));
        return r == VPBS_AGG_OK ? 1 : 0;
    };
    if (reason) *reason = VPBS_AGG_MALFORMED;
    if (!shape_ok(shape) || !bytes) return report(why, why_len, "vpbs_verify_aggregate: null or malformed shape, or null bytes"), VPBS_ERR_INVALID;
    const Statement s{shape->N, shape->K, shape->n_lwe, shape->vks, count, testvs, n_testv, testv_of, cts, out_cts, key_hashes, n_keys, key_of};
    std::string msg;
    if (!statement_ok(s, "vpbs_verify_aggregate", &msg)) return report(why, why_len, msg), VPBS_ERR_INVALID;
    const unsigned d = depth_of(count);
    if (d > shape->levels)
        return report(why, why_len, "vpbs_verify_aggregate: count " + std::to_string(count) + " exceeds 2^levels = " +
                                        std::to_string((size_t)1 << shape->levels)), VPBS_ERR_INVALID;
    vpbs_verify_inputs c = level_inputs(*shape, d);
    if (c.cap_height != 4) return report(why, why_len, "vpbs_verify_aggregate: the level circuits have cap_height 4"), VPBS_ERR_INVALID;
    const size_t n_pi = 4 + VK * d, cap_words = (size_t)4 << c.cap_height;
    std::vector<u64> caps(3 * cap_words), openings(openings_words(c)), fri(len / 8 + 8), pis(n_pi);
    if (vpbs_step_proof_from_bytes(&c, bytes, len, caps.data(), openings.data(), fri.data(), pis.data(), n_pi) != (long)n_pi)
        return verdict(VPBS_AGG_MALFORMED);
    if (std::memcmp(pis.data() + 4, shape->vks, 8 * VK * d) != 0) return verdict(VPBS_AGG_VERIFIER_DATA);
    c.public_inputs = pis.data();
    c.n_public_inputs = n_pi;
    const int ok = vpbs_verify_step(&c, caps.data(), openings.data(), fri.data());
    if (ok < 0) return report(why, why_len, "vpbs_verify_aggregate: malformed circuit description"), ok;
    if (ok != 1) return verdict(VPBS_AGG_PROOF);
    u64 root[4];
    if (!root_host(s, root) || std::memcmp(root, pis.data(), 32) != 0) return verdict(VPBS_AGG_ROOT);
    return verdict(VPBS_AGG_OK);
}

int vpbs_aggregator_create(vpbs_ctx* ctx, const vpbs_verify_inputs* leaf, size_t leaf_n_pi, const vpbs_ivc_circuit* levels, unsigned n_levels,
                           vpbs_aggregator** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    report(err, err_len, "");
    auto refuse = [&](const std::string& m) {
        report(err, err_len, "vpbs_aggregator_create: " + m);
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !leaf || !levels || !out || !leaf->constants_sigmas_cap || n_levels == 0 || n_levels > MAX_LEVELS || leaf_n_pi < VK)
        return refuse("malformed arguments");
    if (vpbs_ctx_rate_bits(ctx) != 3 || vpbs_ctx_cap_height(ctx) != 4 || leaf->rate_bits != 3 || leaf->cap_height != 4)
        return refuse("aggregation needs a context and proofs with rate_bits = 3 and cap_height = 4 (standard_recursion_config)");
    for (unsigned l = 0; l < n_levels; ++l)
        if (!levels[l].circuit || !levels[l].preset_pos || !levels[l].pi_pos) return refuse("level " + std::to_string(l + 1) + ": null circuit, preset_pos or pi_pos");
    auto* a = new vpbs_aggregator();
    a->ctx = ctx;
    a->leaf = *leaf;
    a->leaf.fri_only = 0;
    a->leaf.public_inputs = nullptr;
    a->leaf.n_public_inputs = 0;
    a->leaf.compat = nullptr;
    if (leaf->gates) {
        a->leaf_gates.assign(leaf->gates, leaf->gates + leaf->n_gates);
        a->leaf.gates = a->leaf_gates.data();
    }
    a->vk0.assign(leaf->circuit_digest, leaf->circuit_digest + 4);
    a->vk0.insert(a->vk0.end(), leaf->constants_sigmas_cap, leaf->constants_sigmas_cap + VK - 4);
    a->leaf.constants_sigmas_cap = a->vk0.data() + 4;
    a->leaf_n_pi = leaf_n_pi;
    a->levels.resize(n_levels);
    std::string msg;
    int rc = VPBS_OK;
    size_t inner_words = 0, inner_pi = leaf_n_pi;
    for (unsigned l = 1; l <= n_levels && rc == 0; ++l) {
        Level& L = a->levels[l - 1];
        const vpbs_ivc_circuit& d = levels[l - 1];
        if (d.n_pi != 4 + VK * l || d.n_preset != 2 * (d.proof_words + inner_pi) + VK * l || (l > 1 && d.proof_words != inner_words)) {
            msg = "level " + std::to_string(l) + ": not the aggregation circuit of this level (public inputs / PartialWitness layout / inner proof words)";
            rc = VPBS_ERR_INVALID;
            break;
        }
        rc = L.init(ctx, d, msg);
        if (rc != 0) msg = "level " + std::to_string(l) + ": " + msg;
        L.inner_pi = inner_pi;
        inner_words = L.proof_words();
        inner_pi = L.n_pi;
        a->wire_words = std::max(a->wire_words, (size_t)L.n_wires * L.n);
    }
    if (rc == 0) {
        a->leaf_words = a->levels[0].inner_words;
        const size_t lw = 3 * ((size_t)4 << 4) + openings_words(a->leaf);
        if (a->leaf_words <= lw) {
            msg = "level 1: the inner proof is shorter than the leaf circuit's caps and openings";
            rc = VPBS_ERR_INVALID;
        }
    }
    if (rc == 0) {
        for (auto& b : a->bufs)
            if (!(b = static_cast<u64*>(vpbs_host_alloc(8 * a->wire_words)))) rc = VPBS_ERR_OOM;
        if (rc == 0) rc = vpbs_device_alloc(ctx, a->wire_words, &a->d_wires);
        if (rc != 0) msg = "wire matrices: out of (pinned or device) memory";
    }
    if (rc != 0) {
        report(err, err_len, "vpbs_aggregator_create: " + msg);
        delete a;
        return rc;
    }
    *out = a;
    return VPBS_OK;
}

int vpbs_aggregator_verifier_data(const vpbs_aggregator* a, uint64_t* out) {
    if (!a || !out) return VPBS_ERR_INVALID;
    std::memcpy(out, a->vk0.data(), 8 * VK);
    for (size_t l = 0; l < a->levels.size(); ++l) std::memcpy(out + VK * (l + 1), a->levels[l].vk.data(), 8 * VK);
    return VPBS_OK;
}

int vpbs_aggregator_last_run(const vpbs_aggregator* a, vpbs_aggregate_stats* out) {
    if (!a || !out) return VPBS_ERR_INVALID;
    *out = a->last;
    return VPBS_OK;
}

void vpbs_aggregator_free(vpbs_aggregator* a) { delete a; }

long vpbs_aggregator_run(vpbs_aggregator* a, const uint8_t* bytes, const size_t* offsets, size_t count, uint8_t* out, size_t capacity,
                         vpbs_aggregate_stats* stats, char* err, size_t err_len) {
    report(err, err_len, "");
    if (stats) *stats = vpbs_aggregate_stats{};
    auto fail = [&](long rc, const std::string& m) {
        report(err, err_len, "vpbs_aggregator_run: " + m);
        if (stats && a) *stats = a->last;
        return rc;
    };
    if (!a) return fail(VPBS_ERR_INVALID, "null aggregator");
    std::lock_guard<std::mutex> lock(a->mu);
    reset_stats(a);
    if (!bytes || !offsets || !out) return fail(VPBS_ERR_INVALID, "null bytes, offsets or out");
    if (count == 0) return fail(VPBS_ERR_INVALID, "count is 0: there is nothing to aggregate");
    if (depth_of(count) > a->levels.size())
        return fail(VPBS_ERR_INVALID, "count " + std::to_string(count) + " exceeds 2^levels = " + std::to_string((size_t)1 << a->levels.size()));
    std::string msg;
    long written = 0;   // the one root's bytes go straight into out
    const long rc = run_body(a, bytes, offsets, &count, 1, false,
                             [&](size_t, const Level& L, const Proof& p) { return written = root_bytes(a, L, p, out, capacity, msg); }, msg);
    if (rc < 0) return fail(rc, msg);
    if (stats) *stats = a->last;
    return written;
}

int vpbs_aggregate_level_jobs(const size_t* counts, size_t n_trees, unsigned level, uint32_t* tree, uint32_t* left, uint32_t* right,
                              size_t capacity) {
    if (!counts || n_trees == 0 || level == 0 || (capacity && (!tree || !left || !right))) return VPBS_ERR_INVALID;
    size_t leaves = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        if (counts[t] == 0 || counts[t] > 0xffffffffull - leaves) return VPBS_ERR_INVALID;
        leaves += counts[t];
    }
    const size_t n = level_jobs(counts, n_trees, level, tree, left, right, capacity);
    return n > 0x7fffffffull ? VPBS_ERR_INVALID : (int)n;
}

int vpbs_aggregator_set_device_witness(vpbs_aggregator* a, unsigned max_nodes, char* err, size_t err_len) {
    report(err, err_len, "");
    auto refuse = [&](const std::string& m) {
        report(err, err_len, "vpbs_aggregator_set_device_witness: " + m);
        return VPBS_ERR_INVALID;
    };
    if (!a) return refuse("null aggregator");
    if (max_nodes > (1u << 16)) return refuse("max_nodes must be 0 .. 2^16");
    std::lock_guard<std::mutex> lock(a->mu);
    a->device_witness_off();
    if (max_nodes == 0) return VPBS_OK;
    vpbs_ctx* ctx = a->ctx;
    std::string why;
    for (size_t l = 0; l < a->levels.size() && why.empty(); ++l) {
        Level& L = a->levels[l];
        if (vpbs_witness_device_create(ctx, L.plan, max_nodes, &L.wd) != 0) why = "level " + std::to_string(l + 1) + ": " + vpbs_last_error(ctx);
        a->row_words_max = std::max(a->row_words_max, L.inner_words + L.inner_pi);
    }
    if (why.empty()) {
        try {
            VPBS_HIP(hipSetDevice(ctx->device));
            // at most 2 max_nodes distinct children per chunk, and one word per node for its pair of rows
            const size_t words = (2 * a->row_words_max + 1) * (size_t)max_nodes;
            VPBS_HIP(hipHostMalloc(reinterpret_cast<void**>(&a->h_rows), 8 * words, hipHostMallocDefault));
            for (auto& e : a->ev) VPBS_HIP(hipEventCreate(&e));
            std::vector<u64> vks((a->levels.size() + 1) * VK);
            vpbs_aggregator_verifier_data(a, vks.data());
            if (vpbs_device_alloc(ctx, words, &a->d_rows) != 0 || vpbs_device_alloc(ctx, vks.size(), &a->d_vks) != 0 ||
                vpbs_device_upload(ctx, a->d_vks, vks.data(), vks.size()) != 0)
                why = std::string("child rows and verifier data on the device: ") + vpbs_last_error(ctx);
        } catch (const DeviceError& e) {
            why = e.what;
        }
    }
    if (!why.empty()) {
        a->device_witness_off();
        return refuse(why + "; the aggregator stays on the host path");
    }
    a->max_nodes = max_nodes;
    return VPBS_OK;
}

int vpbs_aggregator_device_stats(const vpbs_aggregator* a, uint64_t out[4]) {
    if (!a || !out) return VPBS_ERR_INVALID;
    std::memcpy(out, a->dev_stats, sizeof a->dev_stats);
    return VPBS_OK;
}

long vpbs_aggregator_run_many(vpbs_aggregator* a, const uint8_t* bytes, const size_t* offsets, const size_t* counts, size_t n_trees,
                              vpbs_aggregate_tree_fn fn, void* user, char* err, size_t err_len) {
    report(err, err_len, "");
    auto fail = [&](long rc, const std::string& m) {
        report(err, err_len, "vpbs_aggregator_run_many: " + m);
        return rc;
    };
    if (!a) return fail(VPBS_ERR_INVALID, "null aggregator");
    std::lock_guard<std::mutex> lock(a->mu);
    reset_stats(a);
    if (n_trees == 0) return fail(VPBS_ERR_INVALID, "n_trees is 0: there is nothing to aggregate");
    if (!bytes || !offsets || !counts || !fn) return fail(VPBS_ERR_INVALID, "null bytes, offsets, counts or fn");
    size_t total = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        if (counts[t] == 0) return fail(VPBS_ERR_INVALID, "tree " + std::to_string(t) + " is empty");
        if (counts[t] > ((size_t)1 << a->levels.size()))
            return fail(VPBS_ERR_INVALID, "tree " + std::to_string(t) + ": count " + std::to_string(counts[t]) + " exceeds 2^levels = " +
                                              std::to_string((size_t)1 << a->levels.size()));
        if (counts[t] > 0xffffffffull - total) return fail(VPBS_ERR_INVALID, "2^32 leaves or more");
        total += counts[t];
        a->last.depth = std::max(a->last.depth, depth_of(counts[t]));   // a refused call reports the depths it saw
    }
    std::string msg;
    // A root is serialised when its tree is through.  The tree whose turn it is goes to fn at once -- on the host path, where the trees come
    // in order, every one; on the device path a shallow tree is through first and is kept until every tree before it has been handed on.
    std::vector<uint8_t> agg(vpbs::aggregator_max_bytes(a));
    std::vector<std::vector<uint8_t>> kept(n_trees);
    std::vector<uint8_t> ready(n_trees, 0);
    size_t handed = 0;
    auto root = [&](size_t t, const Level& L, const Proof& p) {
        const long n = root_bytes(a, L, p, agg.data(), agg.size(), msg);
        if (n < 0) return n;
        if (t != handed) {
            kept[t].assign(agg.begin(), agg.begin() + n);
            ready[t] = 1;
            return n;
        }
        fn(user, handed++, agg.data(), (size_t)n);
        for (; handed < n_trees && ready[handed]; ++handed) {
            fn(user, handed, kept[handed].data(), kept[handed].size());
            std::vector<uint8_t>().swap(kept[handed]);
        }
        return n;
    };
    const long rc = run_body(a, bytes, offsets, counts, n_trees, true, root, msg);
    if (rc < 0) return fail(rc, msg);
    return (long)n_trees;
}

// test_entries.h: the preset matrix of a chunk as the device path assembles it, copied to the host
int vpbs_test_aggregator_preset_matrix(vpbs_aggregator* a, unsigned level, const uint64_t* rows, size_t n_rows, const uint32_t* pairs, unsigned batch,
                                       uint64_t* out) {
    if (!a || !rows || !pairs || !out || level == 0 || level > a->levels.size() || n_rows == 0 || batch == 0) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(a->mu);
    if (batch > a->max_nodes || n_rows > 2 * (size_t)batch) return VPBS_ERR_INVALID;
    for (unsigned j = 0; j < 2 * batch; ++j)
        if (pairs[j] >= n_rows) return VPBS_ERR_INVALID;
    const Level& L = a->levels[level - 1];
    const size_t row_words = L.inner_words + L.inner_pi;
    vpbs_ctx* ctx = a->ctx;
    std::vector<Proof> held(n_rows);
    std::vector<const Proof*> ptrs;
    for (size_t r = 0; r < n_rows; ++r) {
        held[r].flat.assign(rows + r * row_words, rows + r * row_words + L.inner_words);
        held[r].pis.assign(rows + r * row_words + L.inner_words, rows + (r + 1) * row_words);
        ptrs.push_back(&held[r]);
    }
    u64* d_m = nullptr;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const size_t words = L.n_preset * batch;
        d_m = ctx->alloc_words(words);
        VPBS_HIP(hipMemsetAsync(d_m, 0xA5, 8 * words, ctx->stream));   // a word the kernel leaves out shows
        PresetJob job = presets_upload(a, L, level, ptrs, pairs, batch);
        rc = presets_fill(&job, ctx->stream, d_m);
        VPBS_HIP(hipMemcpyAsync(out, d_m, 8 * words, hipMemcpyDeviceToHost, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        (void)vpbs::stream_sync(ctx->stream);
        ctx->err = e.what;
        rc = e.status;
    }
    if (d_m) ctx->release(d_m);
    return rc;
}

int vpbs_aggregate_verifier_create(vpbs_ctx* ctx, const vpbs_aggregate_shape* shape, size_t max_leaves, vpbs_aggregate_verifier** out, char* err,
                                   size_t err_len) {
    return vpbs_aggregate_verifier_create_many(ctx, shape, max_leaves, 1, out, err, err_len);
}

int vpbs_aggregate_verifier_create_many(vpbs_ctx* ctx, const vpbs_aggregate_shape* shape, size_t max_leaves, size_t max_aggregates,
                                        vpbs_aggregate_verifier** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    report(err, err_len, "");
    auto refuse = [&](const char* m) {
        report(err, err_len, std::string("vpbs_aggregate_verifier_create: ") + m);
        return VPBS_ERR_INVALID;
    };
    if (max_aggregates == 0 || max_aggregates > (1u << 16)) return refuse("max_aggregates must be 1 .. 2^16");
    if (!ctx || !out || !shape_ok(shape)) return refuse("null or malformed arguments");
    if (shape->N == 0 || shape->K == 0 || (size_t)shape->K * shape->N > (1u << 20) || shape->n_lwe > (1u << 24)) return refuse("N, K or n_lwe out of range");
    if (max_leaves == 0 || max_leaves > (1u << 20)) return refuse("max_leaves must be 1 .. 2^20");
    for (unsigned l = 1; l <= shape->levels; ++l)
        if (shape->level_shapes[l - 1].cap_height != 4) return refuse("the level circuits have cap_height 4");
    auto* v = new vpbs_aggregate_verifier;
    v->N = shape->N; v->K = shape->K; v->n_lwe = shape->n_lwe;
    v->max_leaves = max_leaves;
    v->max_aggregates = max_aggregates;
    // only the levels max_leaves can reach get a batch verifier
    v->levels = std::min(shape->levels, depth_of(max_leaves));
    for (unsigned l = 1; l <= v->levels; ++l) {
        const vpbs_verify_inputs c = level_inputs(*shape, l);
        vpbs_proof_verifier* p = nullptr;
        const int rc = vpbs_proof_verifier_create(ctx, &c, max_aggregates, 4 + VK * l, &p, err, err_len);
        if (rc) {
            delete v;
            return rc;
        }
        v->proofs.push_back(p);
    }
    v->ctx = ctx;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        v->d_vks = static_cast<u64*>(v->alloc(8 * VK * (v->levels + 1)));
        v->d_in = static_cast<u64*>(v->alloc(8 * v->in_words()));
        v->d_stmt = static_cast<u64*>(v->alloc(32 * max_leaves));
        VPBS_HIP(hipHostMalloc((void**)&v->h_in, 8 * v->in_words(), hipHostMallocDefault));
        for (auto& n : v->d_mnodes) n = static_cast<u64*>(v->alloc(32 * max_leaves));
        v->d_roots = static_cast<u64*>(v->alloc(32 * max_aggregates));
        v->d_mflags = static_cast<u32*>(v->alloc(4 * max_aggregates));
        v->d_midx = static_cast<u32*>(v->alloc(4 * v->many_idx_words()));
        v->d_mout = static_cast<uint8_t*>(v->alloc(2 * max_aggregates));
        VPBS_HIP(hipHostMalloc((void**)&v->h_midx, 4 * v->many_idx_words(), hipHostMallocDefault));
        VPBS_HIP(hipHostMalloc((void**)&v->h_mout, 40 * max_aggregates, hipHostMallocDefault));
        VPBS_HIP(hipMemcpyAsync(v->d_vks, shape->vks, 8 * VK * (v->levels + 1), hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        delete v;
        return e.status;
    }
    *out = v;
    return VPBS_OK;
}

void vpbs_aggregate_verifier_free(vpbs_aggregate_verifier* v) { delete v; }

}  // extern "C"

// ================= the device verifier's runs: the trees of a run, one or many =================
namespace {
// what run and root refuse, by name, before anything is queued
bool verifier_args_ok(vpbs_aggregate_verifier* v, const Statement& s, const char* who, std::string* msg) {
    if (!statement_ok(s, who, msg)) return false;
    if (s.count > v->max_leaves || s.n_testv > v->max_leaves || s.n_keys > v->max_leaves) {
        *msg = std::string(who) + ": count, n_testv or n_keys exceeds max_leaves " + std::to_string(v->max_leaves);
        return false;
    }
    if (depth_of(s.count) > v->levels) {
        *msg = std::string(who) + ": count " + std::to_string(s.count) + " exceeds 2^levels = " + std::to_string((size_t)1 << v->levels);
        return false;
    }
    return true;
}

// What run_many and roots_many refuse, by name, before anything is queued; s.count is the total leaf count.  depth: of every tree.
bool many_args_ok(vpbs_aggregate_verifier* v, const Statement& s, size_t n_agg, const size_t* leaf_first, const char* who, std::vector<unsigned>* depth,
                  std::string* msg) {
    auto no = [&](const std::string& m) {
        *msg = std::string(who) + ": " + m;
        return false;
    };
    if (n_agg == 0) return no("n_agg is 0: there is nothing to verify");
    if (!leaf_first) return no("null leaf_first");
    if (n_agg > v->max_aggregates) return no("n_agg " + std::to_string(n_agg) + " exceeds max_aggregates " + std::to_string(v->max_aggregates));
    if (leaf_first[0] != 0) return no("leaf_first[0] must be 0");
    depth->assign(n_agg, 0);
    for (size_t a = 0; a < n_agg; ++a) {
        if (leaf_first[a + 1] <= leaf_first[a]) return no("tree " + std::to_string(a) + " is empty (leaf_first must increase)");
        const size_t count = leaf_first[a + 1] - leaf_first[a];
        if (count > ((size_t)1 << v->levels))
            return no("tree " + std::to_string(a) + ": " + std::to_string(count) + " leaves exceed 2^levels = " + std::to_string((size_t)1 << v->levels));
        (*depth)[a] = depth_of(count);
    }
    if (leaf_first[n_agg] != s.count) return no("leaf_first ends at " + std::to_string(leaf_first[n_agg]) + ", not at the leaf count");
    if (s.count > v->max_leaves || s.n_testv > v->max_leaves || s.n_keys > v->max_leaves)
        return no("the leaf count " + std::to_string(s.count) + ", n_testv or n_keys exceeds max_leaves " + std::to_string(v->max_leaves));
    return statement_ok(s, who, msg);
}

// The statement stages of all trees, queued on the context's stream: ag_leaf_pair over all leaves, then one ag_fold_many per level over the
// trees that have that level.  After them d_roots [n_agg][4] holds the roots and d_mflags [n_agg] the raw-word flags.  *agg_idx: where the
// caller may put further u32 tables in h_midx / d_midx (the upload of h_midx is the caller's, before its first launch that reads them; the
// tables of this function are uploaded here).
void many_statement_enqueue(vpbs_aggregate_verifier* v, const Statement& s, size_t n_agg, const size_t* leaf_first, const std::vector<unsigned>& depth,
                            int on_device, size_t extra_idx, size_t* agg_idx) {
    vpbs_ctx* ctx = v->ctx;
    hipStream_t st = ctx->stream;
    const size_t total = s.count, kn = v->kn();
    const size_t n_ct = total * ((size_t)s.n_lwe + 1), n_out = total * kn, n_tv = s.n_testv * (size_t)s.N, n_kh = 4 * s.n_keys;
    const u64 *d_ct = s.cts, *d_oc = s.out_cts, *d_tv = s.testvs, *d_kh = s.key_hashes;
    if (!on_device) {
        std::memcpy(v->h_in, s.cts, 8 * n_ct);
        std::memcpy(v->h_in + n_ct, s.out_cts, 8 * n_out);
        std::memcpy(v->h_in + n_ct + n_out, s.testvs, 8 * n_tv);
        std::memcpy(v->h_in + n_ct + n_out + n_tv, s.key_hashes, 8 * n_kh);
        VPBS_HIP(hipMemcpyAsync(v->d_in, v->h_in, 8 * (n_ct + n_out + n_tv + n_kh), hipMemcpyHostToDevice, st));
        d_ct = v->d_in;
        d_oc = v->d_in + n_ct;
        d_tv = v->d_in + n_ct + n_out;
        d_kh = v->d_in + n_ct + n_out + n_tv;
    }
    // ---- the index tables, computed once per run ----
    u32* idx = v->h_midx;
    unsigned max_d = 0;
    for (size_t a = 0; a < n_agg; ++a) {
        max_d = std::max(max_d, depth[a]);
        for (size_t i = leaf_first[a]; i < leaf_first[a + 1]; ++i) {
            idx[i] = (u32)s.tv(i);
            idx[total + i] = (u32)s.key(i);
            idx[2 * total + i] = (u32)a;
        }
    }
    size_t at = 3 * total;
    std::vector<size_t> o_tree(max_d + 1), o_tab(max_d + 1), nodes(max_d + 1, 0);
    std::vector<u32> prev_first(n_agg), prev_n(n_agg);   // the tree's entries in the level below
    for (size_t a = 0; a < n_agg; ++a) {
        prev_first[a] = (u32)leaf_first[a];
        prev_n[a] = (u32)(leaf_first[a + 1] - leaf_first[a]);
    }
    for (unsigned l = 1; l <= max_d; ++l) {
        o_tree[l] = at;
        u32 node = 0;
        std::vector<FoldTree> tab(n_agg, FoldTree{0, 1, 0, 0});
        for (size_t a = 0; a < n_agg; ++a) {
            if (depth[a] < l) continue;
            const u32 mine = 1u << (depth[a] - l);
            tab[a] = FoldTree{prev_first[a], prev_n[a], node, depth[a] == l ? 1u : 0u};
            for (u32 k = 0; k < mine; ++k) idx[at + node + k] = (u32)a;
            prev_first[a] = node;
            prev_n[a] = mine;
            node += mine;
        }
        nodes[l] = node;
        at += node;
        o_tab[l] = at;
        std::memcpy(idx + at, tab.data(), sizeof(FoldTree) * n_agg);
        at += 4 * n_agg;
    }
    *agg_idx = at;
    VPBS_REQUIRE(at + extra_idx <= v->many_idx_words(), "the index tables of the run exceed their buffer");
    VPBS_HIP(hipMemcpyAsync(v->d_midx, v->h_midx, 4 * at, hipMemcpyHostToDevice, st));
    VPBS_HIP(hipMemsetAsync(v->d_mflags, 0, 4 * n_agg, st));
    const AggShape S{s.N, (u32)kn, s.n_lwe, (u32)s.n_pi()};
    {
        vpbs::Timed t(ctx, "ag_leaf_pair");
        ag_leaf_pair<<<(u32)total, 32, 0, st>>>(d_tv, v->d_midx, d_oc, d_kh, v->d_midx + total, d_ct, v->d_vks, v->d_midx + 2 * total, S, v->d_stmt,
                                                v->d_mflags);
    }
    VPBS_HIP(hipGetLastError());
    {
        vpbs::Timed t(ctx, "ag_fold_many");
        const u64* in = v->d_stmt;
        for (unsigned l = 1; l <= max_d; ++l) {
            u64* out = v->d_mnodes[l & 1];
            ag_fold_many<<<(u32)nodes[l], 16, 0, st>>>(in, v->d_midx + o_tree[l], reinterpret_cast<const FoldTree*>(v->d_midx + o_tab[l]), out, v->d_roots);
            in = out;
        }
    }
    VPBS_HIP(hipGetLastError());
}

// ---- The two cores of the four entry points, under the verifier's lock: s, n_agg, leaf_first and depth are through the entry point's own
// refusals, `who` names it in what a core reports.  Everything from the statement stages to the one wait, and the read-back. ----

// the statement stages alone -> out [n_agg][4] and raw_bad [n_agg]; VPBS_OK, or < 0 with err
int roots_core(vpbs_aggregate_verifier* v, const Statement& s, size_t n_agg, const size_t* leaf_first, const std::vector<unsigned>& depth,
               int on_device, const char* who, uint64_t* out, uint8_t* raw_bad, char* err, size_t err_len) {
    try {
        VPBS_HIP(hipSetDevice(v->ctx->device));
        hipStream_t st = v->ctx->stream;
        size_t at = 0;
        many_statement_enqueue(v, s, n_agg, leaf_first, depth, on_device, 0, &at);
        VPBS_HIP(hipMemcpyAsync(v->h_mout, v->d_roots, 32 * n_agg, hipMemcpyDeviceToHost, st));
        VPBS_HIP(hipMemcpyAsync(v->h_mout + 4 * n_agg, v->d_mflags, 4 * n_agg, hipMemcpyDeviceToHost, st));
        VPBS_HIP(vpbs::stream_sync(st));   // the one wait
    } catch (const DeviceError& e) {
        v->ctx->err = e.what;
        return report(err, err_len, std::string(who) + ": " + e.what), e.status;
    }
    std::memcpy(out, v->h_mout, 32 * n_agg);
    const u32* flags = reinterpret_cast<const u32*>(v->h_mout + 4 * n_agg);
    for (size_t a = 0; a < n_agg; ++a) raw_bad[a] = flags[a] ? 1 : 0;
    return VPBS_OK;
}

// aggregate a = bytes[offsets[a] .. offsets[a + 1]) against tree a -> verdicts [n_agg], reasons [n_agg] (may be null); the number accepted,
// or < 0 with err
long run_core(vpbs_aggregate_verifier* v, const Statement& s, const uint8_t* bytes, const size_t* offsets, size_t n_agg, const size_t* leaf_first,
              const std::vector<unsigned>& depth, int on_device, const char* who, uint8_t* verdicts, uint8_t* reasons, char* err, size_t err_len) {
    try {
        VPBS_HIP(hipSetDevice(v->ctx->device));
        hipStream_t st = v->ctx->stream;
        size_t at = 0;
        many_statement_enqueue(v, s, n_agg, leaf_first, depth, on_device, n_agg, &at);
        // agg_of: the aggregates grouped by depth, each depth ONE batch of its level's proof verifier
        std::vector<std::vector<u32>> of_depth(v->levels + 1);
        for (size_t a = 0; a < n_agg; ++a) of_depth[depth[a]].push_back((u32)a);
        u32* agg_of = v->h_midx + at;
        size_t k = 0;
        for (unsigned d = 1; d <= v->levels; ++d)
            for (u32 a : of_depth[d]) agg_of[k++] = a;
        VPBS_HIP(hipMemcpyAsync(v->d_midx + at, agg_of, 4 * n_agg, hipMemcpyHostToDevice, st));
        std::vector<uint8_t> packed;
        std::vector<size_t> offs;
        size_t first = 0;
        for (unsigned d = 1; d <= v->levels; ++d) {
            const std::vector<u32>& mine = of_depth[d];
            if (mine.empty()) continue;
            packed.clear();
            offs.assign(1, 0);
            for (u32 a : mine) {
                packed.insert(packed.end(), bytes + offsets[a], bytes + offsets[a + 1]);
                offs.push_back(packed.size());
            }
            if (packed.empty()) packed.push_back(0);   // a valid pointer for a batch of empty blobs
            vpbs::ProofBatchView pv{};
            const int rc = vpbs::proof_verifier_enqueue(v->proofs[d - 1], packed.data(), offs.data(), mine.size(), &pv);
            if (rc) {
                (void)vpbs::stream_sync(st);
                return report(err, err_len, std::string(who) + ": the batch verifier refused the bytes"), (long)rc;
            }
            const u32 n_expected = (u32)(4 + VK * d), n = (u32)mine.size();
            VPBS_REQUIRE(pv.max_pi >= n_expected, "the batch verifier's slot is smaller than the aggregate's public inputs");
            ag_result_many<<<(n + 63) / 64, 64, 0, st>>>(pv.reasons, pv.n_pi, pv.words, pv.W, pv.n_fixed, v->d_vks, v->d_roots, v->d_mflags,
                                                         v->d_midx + at + first, n, n_expected, v->d_mout);
            VPBS_HIP(hipGetLastError());
            first += mine.size();
        }
        VPBS_HIP(hipMemcpyAsync(v->h_mout, v->d_mout, 2 * n_agg, hipMemcpyDeviceToHost, st));
        VPBS_HIP(vpbs::stream_sync(st));   // the one wait
    } catch (const DeviceError& e) {
        v->ctx->err = e.what;
        return report(err, err_len, std::string(who) + ": " + e.what), (long)e.status;
    }
    const uint8_t* o = reinterpret_cast<const uint8_t*>(v->h_mout);
    long accepted = 0;
    for (size_t a = 0; a < n_agg; ++a) {
        verdicts[a] = o[2 * a];
        if (reasons) reasons[a] = o[2 * a + 1];
        accepted += o[2 * a];
    }
    return accepted;
}

const u64 VK0_ON_DEVICE = 0;   // the host checks of a Statement need a non-null vk0; the device holds the real one
}  // namespace

namespace vpbs {
unsigned aggregator_levels(const vpbs_aggregator* a) { return (unsigned)a->levels.size(); }
unsigned aggregator_device_witness(const vpbs_aggregator* a) { return a->max_nodes; }
size_t aggregator_max_bytes(const vpbs_aggregator* a) {
    size_t most = 0;
    for (const Level& L : a->levels) most = std::max(most, 8 * ((size_t)L.n_wires * 64 + ((size_t)1 << 17)) + 8 * L.n_pi);
    return most;
}
void aggregate_verifier_shape(const vpbs_aggregate_verifier* v, AggregateVerifierShape* out) {
    *out = AggregateVerifierShape{v->ctx, v->N, v->K, v->n_lwe, v->levels, v->max_leaves, v->max_aggregates};
}
}  // namespace vpbs

extern "C" {
int vpbs_aggregate_verifier_roots_many(vpbs_aggregate_verifier* v, size_t n_agg, const size_t* leaf_first, const uint64_t* testvs, size_t n_testv,
                                       const uint32_t* testv_of, const uint64_t* cts, const uint64_t* out_cts, const uint64_t* key_hashes,
                                       size_t n_keys, const uint32_t* key_of, int on_device, uint64_t* out, uint8_t* raw_bad, char* err,
                                       size_t err_len) {
    report(err, err_len, "");
    const char* who = "vpbs_aggregate_verifier_roots_many";
    if (!v || !out || !raw_bad) return report(err, err_len, std::string(who) + ": null argument"), VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    const Statement s{v->N, v->K, v->n_lwe, &VK0_ON_DEVICE, leaf_first && n_agg ? leaf_first[n_agg] : 0, testvs, n_testv, testv_of, cts, out_cts,
                      key_hashes, n_keys, key_of};
    std::string msg;
    std::vector<unsigned> depth;
    if (!many_args_ok(v, s, n_agg, leaf_first, who, &depth, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    return roots_core(v, s, n_agg, leaf_first, depth, on_device, who, out, raw_bad, err, err_len);
}

long vpbs_aggregate_verifier_run_many(vpbs_aggregate_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t n_agg, const size_t* leaf_first,
                                      const uint64_t* testvs, size_t n_testv, const uint32_t* testv_of, const uint64_t* cts, const uint64_t* out_cts,
                                      const uint64_t* key_hashes, size_t n_keys, const uint32_t* key_of, int on_device, uint8_t* verdicts,
                                      uint8_t* reasons, char* err, size_t err_len) {
    report(err, err_len, "");
    const char* who = "vpbs_aggregate_verifier_run_many";
    if (!v || !bytes || !offsets || !verdicts) return report(err, err_len, std::string(who) + ": null argument"), VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    const Statement s{v->N, v->K, v->n_lwe, &VK0_ON_DEVICE, leaf_first && n_agg ? leaf_first[n_agg] : 0, testvs, n_testv, testv_of, cts, out_cts,
                      key_hashes, n_keys, key_of};
    std::string msg;
    std::vector<unsigned> depth;
    if (!many_args_ok(v, s, n_agg, leaf_first, who, &depth, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    for (size_t a = 0; a < n_agg; ++a)
        if (offsets[a + 1] < offsets[a]) return report(err, err_len, std::string(who) + ": offsets decrease at aggregate " + std::to_string(a)), VPBS_ERR_INVALID;
    return run_core(v, s, bytes, offsets, n_agg, leaf_first, depth, on_device, who, verdicts, reasons, err, err_len);
}

// ---- one tree: the same cores behind the single entry points' own refusals ----
int vpbs_aggregate_verifier_root(vpbs_aggregate_verifier* v, size_t count, const uint64_t* testvs, size_t n_testv, const uint32_t* testv_of,
                                 const uint64_t* cts, const uint64_t* out_cts, const uint64_t* key_hashes, size_t n_keys, const uint32_t* key_of,
                                 int on_device, uint64_t out[4], char* err, size_t err_len) {
    report(err, err_len, "");
    const char* who = "vpbs_aggregate_verifier_root";
    if (!v || !out) return report(err, err_len, std::string(who) + ": null argument"), VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    const Statement s{v->N, v->K, v->n_lwe, &VK0_ON_DEVICE, count, testvs, n_testv, testv_of, cts, out_cts, key_hashes, n_keys, key_of};
    std::string msg;
    if (!verifier_args_ok(v, s, who, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    const size_t leaf_first[2] = {0, count};
    u64 root[4];
    uint8_t raw_bad = 0;
    const int rc = roots_core(v, s, 1, leaf_first, {depth_of(count)}, on_device, who, root, &raw_bad, err, err_len);
    if (rc != VPBS_OK) return rc;
    if (raw_bad) return 1;
    std::memcpy(out, root, 32);
    return VPBS_OK;
}

int vpbs_aggregate_verifier_run(vpbs_aggregate_verifier* v, const uint8_t* bytes, size_t len, size_t count, const uint64_t* testvs, size_t n_testv,
                                const uint32_t* testv_of, const uint64_t* cts, const uint64_t* out_cts, const uint64_t* key_hashes, size_t n_keys,
                                const uint32_t* key_of, int on_device, int* reason, char* err, size_t err_len) {
    report(err, err_len, "");
    const char* who = "vpbs_aggregate_verifier_run";
    if (reason) *reason = VPBS_AGG_MALFORMED;
    if (!v || !bytes) return report(err, err_len, std::string(who) + ": null argument"), VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    const Statement s{v->N, v->K, v->n_lwe, &VK0_ON_DEVICE, count, testvs, n_testv, testv_of, cts, out_cts, key_hashes, n_keys, key_of};
    std::string msg;
    if (!verifier_args_ok(v, s, who, &msg)) return report(err, err_len, msg), VPBS_ERR_INVALID;
    const size_t leaf_first[2] = {0, count}, offsets[2] = {0, len};
    uint8_t verdict = 0, why = VPBS_AGG_MALFORMED;
    const long rc = run_core(v, s, bytes, offsets, 1, leaf_first, {depth_of(count)}, on_device, who, &verdict, &why, err, err_len);
    if (rc < 0) return (int)rc;
    if (reason) *reason = why;
    return verdict;
}
}  // extern "C"

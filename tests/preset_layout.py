"""The early-phase preset matrix of the device-witness pipeline, stated in numpy from the table of DESIGN.md 8.5: for chain steps
[first, first + cnt) a matrix [n_preset][cnt] (instances innermost) whose rows are, per step s,

    previous proof's words [proof_words]      zeros (late presets: the early phase ignores them)
    public inputs of the predecessor [n_pi]   acc_init = (0, .., 0, testv) | counter s | accumulator accs[s - 1] | key link s - 1 |
                                              LWE link s - 1 | the cyclic circuit's verifier data          (zeros before step 0)
    condition                                 s != 0
    GGSW [ggsw_len]                           zeros, bsk[s - 1], ksk
    mask                                      ct[n], ct[s - 1], 0
    own | dummy verifier data, dummy proof    constants
    the dummy proof's public inputs [n_pi]    zeros

The yardstick for the host loop's matrix (vpbs_test_ivc_preset_matrix) on the CPU and for the kernels of csrc/pbs_prove_batch.hip on the GPU."""
import numpy as np


def lwe_masks(ct):
    """the items of the LWE hash chain / the mask of every step: ct[n], ct[0] .. ct[n - 1], 0"""
    c = np.asarray(ct, np.uint64).reshape(-1)
    return np.concatenate([c[-1:], c[:-1], np.zeros(1, np.uint64)])


def predecessor_public_inputs(s, testv, accs, key_links, lwe_links, cyc_vk, kn):
    """public inputs of the proof step s verifies: the base proof's for s = 0, step s - 1's otherwise"""
    tv = np.asarray(testv, np.uint64).reshape(-1)
    acc_init = np.concatenate([np.zeros(kn - tv.size, np.uint64), tv])
    if s == 0:
        state = np.zeros(1 + kn + 8, np.uint64)
    else:
        state = np.concatenate([np.array([s], np.uint64), np.asarray(accs[s - 1], np.uint64).reshape(-1),
                                np.asarray(key_links[s - 1], np.uint64), np.asarray(lwe_links[s - 1], np.uint64)])
    return np.concatenate([acc_init, state, np.asarray(cyc_vk, np.uint64)])


def matrix(first, cnt, proof_words, testv, accs, key_links, lwe_links, ct, bsk, ksk, cyc_vk, dum_vk, dummy_proof):
    """accs [n + 2][K N], key_links / lwe_links [n + 2][4], ct [n + 1], bsk [n][ggsw_len], ksk [ggsw_len] -> [n_preset][cnt]"""
    ksk = np.asarray(ksk, np.uint64).reshape(-1)
    accs = np.asarray(accs, np.uint64).reshape(len(accs), -1)
    kn, n = accs.shape[1], len(ct) - 1
    masks = lwe_masks(ct)
    cols = []
    for s in range(first, first + cnt):
        pis = predecessor_public_inputs(s, testv, accs, key_links, lwe_links, cyc_vk, kn)
        ggsw = np.zeros(ksk.size, np.uint64) if s == 0 else (np.asarray(bsk[s - 1], np.uint64).reshape(-1) if s <= n else ksk)
        cols.append(np.concatenate([np.zeros(proof_words, np.uint64), pis, np.array([1 if s else 0], np.uint64), ggsw, masks[s:s + 1],
                                    np.asarray(cyc_vk, np.uint64), np.asarray(dum_vk, np.uint64), np.asarray(dummy_proof, np.uint64),
                                    np.zeros(pis.size, np.uint64)]))
    return np.ascontiguousarray(np.stack(cols, axis=1))

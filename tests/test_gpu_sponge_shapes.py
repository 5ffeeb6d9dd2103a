"""GPU tests (-m gpu) of the sponge in the lane-per-permutation hashing kernels (csrc/hash.hip) at every shape of its absorb loop.  The kernels
compute only the rows of the last MDS layer that the sponge reads (poseidon::permute_sponge): the digest's after the last block, the capacity's
where a whole block overwrites the rest, all twelve where a partial block follows.  A row left out by mistake, or a stale word read, changes a
digest -- so every digest word is compared with the CPU oracle, through the entry points of tests/test_gpu_parity.py:
    hash_rows         hash_rows_kernel        any words, taken as residues
    merkle_cap        hash_rows_kernel + merkle_level_kernel (two-to-one: one block, the digest rows only)
    commit_values     leaf_hash_kernel over the LDE + the tree; every leaf digest is a sibling of some opening
    fri_prove         fri_leaf_hash_kernel at arity 16 (four full blocks per leaf)
Column counts: 1 and 4 (one short block; hash-or-noop in a commitment), 5, 7, 8 (one block), 9, 12, 15 (a partial second block of every
critical length: its rows 1, 4 and 7 stay the permutation's), 16, 24 (exact multiples: capacity rows only), 17, 20, 23, 25, 33 and the three
real shapes 135 (wires), 20 (Z / partial products) and 16 (quotient).  Leaf counts 64, 256 and 300 (no multiple of the workgroup).  The context
runs with wide_threshold 0, so that small levels and small FRI trees take the lane form too."""
import numpy as np
import pytest

import oracle as orc
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
NCOLS = [1, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 23, 24, 25, 33, 135]
LEAF_COUNTS = [64, 256, 300]


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    c.set_option("wide_threshold", 0)
    yield c
    c.close()


def _rows(ncols):
    """300 rows: random words of the whole u64 range (residues), then rows of 0, p - 1 and 2^64 - 1, a row that alternates them, canonical rows"""
    rng = np.random.default_rng(1000 + ncols)
    rows = rng.integers(0, 1 << 64, size=(300, ncols), dtype=np.uint64, endpoint=False)
    rows[1], rows[2], rows[3] = 0, P - 1, (1 << 64) - 1
    rows[4] = [(0, P - 1, (1 << 64) - 1, (1 << 32) - 1, 1 << 63)[k % 5] for k in range(ncols)]
    rows[5:64] = rng.integers(0, P, size=(59, ncols), dtype=np.uint64)
    rows[299] = (1 << 64) - 1                                              # the last lane of the partly filled workgroup
    return rows


@pytest.fixture(scope="module")
def digests():
    """oracle digests of the 300 rows of every column count, computed once: hash_n_to_m_no_pad of the words mod p"""
    return {n: np.array([orc.hash_no_pad(r % np.uint64(P)) for r in _rows(n)], dtype=np.uint64) for n in NCOLS}


@pytest.mark.parametrize("ncols", NCOLS)
def test_hash_rows_digests_at_every_absorb_shape(ctx, digests, ncols):
    rows = _rows(ncols)
    for n in LEAF_COUNTS:
        got = ctx.hash_rows(np.ascontiguousarray(rows[:n]))
        assert got.shape == (n, 4)
        bad = np.nonzero((got != digests[ncols][:n]).any(axis=1))[0]
        assert bad.size == 0, (ncols, n, bad[:8].tolist())


@pytest.mark.parametrize("ncols", [5, 9, 16, 17, 20, 135])
@pytest.mark.parametrize("n_leaves,cap_h", [(64, 0), (256, 4)])
def test_merkle_cap_with_every_level_in_the_lane_form(ctx, ncols, n_leaves, cap_h):
    leaves = np.ascontiguousarray(_rows(ncols)[:n_leaves] % np.uint64(P))
    assert (ctx.merkle_cap(leaves, cap_h) == orc.Merkle(leaves, cap_h).cap()).all()


@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("log_n", [3, 5])
def test_commitment_leaf_digests_at_every_absorb_shape(ctx, ncols, log_n):
    """leaf_hash_kernel over 64 and 256 LDE leaves: the cap, and every leaf with its Merkle path (the lowest sibling is the neighbour's leaf
    digest, so every digest word of the kernel is compared)"""
    rng = np.random.default_rng(50 * ncols + log_n)
    data = rng.integers(0, P, size=(ncols, 1 << log_n), dtype=np.uint64)
    data[0] = P - 1
    if ncols > 1:
        data[ncols - 1] = 0
    want = orc.Batch(data, 3, 4, from_values=True)
    got = ctx.commit_values(data)
    try:
        assert (got.cap_at_commit == want.cap()).all() and (got.cap() == want.cap()).all()
        for idx in range(1 << (log_n + 3)):
            leaf, sib = got.open(idx)
            wleaf, wsib = want.open(idx)
            assert (leaf == wleaf).all() and (sib == wsib).all(), (ncols, log_n, idx)
    finally:
        got.free()


def test_fri_leaf_hash_at_arity_16_in_the_lane_form(ctx):
    """the standard FRI configuration folds by 16: a leaf is 32 words, four full blocks -- capacity rows three times, then the digest rows.  With
    wide_threshold 0 the lane form hashes the leaves of every round; the whole proof is compared word for word."""
    from test_gpu_parity import _fri_case
    log_n = 9
    ob, gb, ch, gch, batches, openings, op, gp = _fri_case(ctx, log_n, (4, 6, 3, 2))
    want = orc.prove_openings(ob, batches, ch, op, log_n)
    got = ctx.fri_prove(gb, batches, gch, gp)
    assert got.shape == want.shape and (got == want).all()
    assert gch.state_words() == ch.state_words()

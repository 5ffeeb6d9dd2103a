"""GPU tests (-m gpu) of the rotation margins (vpbs_lwe_rotation_batch, lwe_rotation_batch_kernel; csrc/lwe_client.hip, csrc/rotation.h; DESIGN.md
8.19).  Yardsticks: the same call with a null context (the host form, itself held to the Python restatement by
tests/test_lwe_rotation_cpu.py) word for word, and -- the prediction contract -- the bootstraps themselves: what Bootstrapper.run puts into
the output GLWE is what the call said it would, at every coefficient, on phases that step across every block edge.  Exact integers."""
import numpy as np
import pytest
import torch

import lwe_client_oracle as O
import pbs_batch_oracle as B
import rotation_oracle as R
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
ALL = ("rot", "idx", "dev")
SHAPES = [(1, 0, 1), (3, 2, 2), (7, 3, 128), (10, 1, 2), (11, 3, 2048), (10, 0, 1)]     # log_N, log_slots, p


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_zeros(*shape):
    d = torch.zeros(shape, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()         # torch fills on its stream, the calls work on the context's own
    return d


def back(d):
    return d.cpu().numpy().view(np.uint64)


def same_outputs(got, want, names):
    assert sorted(got) == sorted(names)
    for k in names:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), (k, np.argwhere(got[k] != want[k])[:4].tolist())


@pytest.mark.parametrize("n_lwe", [1, 5, 63, 64, 65, 728])
def test_device_form_is_the_host_form(ctx, n_lwe):
    """the edge rows of the CPU suite in the three modes of vpbs_decode_where, the key on either side; counts 1, 3, 4, 5 end inside and at
    the end of a workgroup's four rows, the full set spans several workgroups"""
    for log_n, theta, p in SHAPES:
        N = 1 << log_n
        rows = R.edge_rows(log_n, n_lwe, theta, 300 + n_lwe)
        keys = R.keys(n_lwe, n_lwe + log_n)                      # all-zero, all-one, mixed: all three at two shapes, the mixed one everywhere
        for s in (keys if (log_n, theta, p) in SHAPES[1:3] else keys[2:]):
            d_s = to_dev(s)
            for count in (1, 3, 4, 5, len(rows)):
                cts = rows[::len(rows) // count][:count]              # spread over the set: edge rows and, from count 3 on, random ones
                expected = np.array([[0, p - 1, p, 2 * p - 1, 2 * p, 2 * p + 3, (1 << 64) - 1][i % 7] for i in range(count)], np.uint64)
                d_cts, d_exp = to_dev(cts), to_dev(expected)
                for exp, d_e in ((None, None), (expected, d_exp)):
                    hst, st0, st2, st1 = api.NoiseStats(), api.NoiseStats(), api.NoiseStats(), api.NoiseStats()
                    want = api.lwe_rotation_batch(s, cts, N, p, log_slots=theta, expected=exp, stats=hst, want=ALL)            # null context
                    same_outputs(ctx.lwe_rotation_batch(s, cts, N, p, log_slots=theta, expected=exp, stats=st0, want=ALL), want, ALL)   # host pointers
                    got = ctx.lwe_rotation_batch(d_s.data_ptr(), d_cts.data_ptr(), N, p, log_slots=theta, expected=None if exp is None else d_e.data_ptr(),
                                                 count=count, stats=st2, want=ALL, n_lwe=n_lwe)                                # outputs to the host
                    same_outputs(got, want, ALL)
                    st2h = api.NoiseStats()                           # the same mode with the key on the host
                    same_outputs(ctx.lwe_rotation_batch(s, d_cts.data_ptr(), N, p, log_slots=theta, expected=exp, count=count, stats=st2h, want=ALL),
                                 want, ALL)
                    d_o = {k: dev_zeros(count) for k in ALL}
                    assert ctx.lwe_rotation_batch(s, d_cts.data_ptr(), N, p, log_slots=theta, expected=exp, count=count, stats=st1,
                                                  want={k: d.data_ptr() for k, d in d_o.items()}) is None                       # all on the device
                    for k in ALL:
                        assert (back(d_o[k]) == want[k].view(np.uint64)).all(), (k, log_n, theta, p, count)
                    d_k, st1d = {k: dev_zeros(count) for k in ALL}, api.NoiseStats()      # device outputs with the key on the device
                    assert ctx.lwe_rotation_batch(d_s.data_ptr(), d_cts.data_ptr(), N, p, log_slots=theta, expected=None if exp is None else d_e.data_ptr(),
                                                  count=count, stats=st1d, want={k: d.data_ptr() for k, d in d_k.items()}, n_lwe=n_lwe) is None
                    for k in ALL:
                        assert (back(d_k[k]) == want[k].view(np.uint64)).all(), (k, log_n, theta, p, count)
                    for st in (st0, st2, st2h, st1, st1d):
                        assert st.as_dict() == hst.as_dict(), (log_n, theta, p, count)
                if count == len(rows):
                    plain = api.lwe_rotation_batch(s, cts, N, p, log_slots=theta, want=ALL)
                    for drop in ALL:                                  # each output pointer NULL in turn, no expected and no statistics
                        names = tuple(k for k in ALL if k != drop)
                        same_outputs(ctx.lwe_rotation_batch(s, d_cts.data_ptr(), N, p, log_slots=theta, count=count, want=names), plain, names)


def test_a_full_grid_and_one_row_more(ctx):
    """8193 rows of n_lwe 5: one past 2048 workgroups of four waves, so the grid stride runs; the tally is the host's"""
    n, count, log_n, p = 5, 4 * 2048 + 1, 7, 2
    rng = np.random.default_rng(17)
    s = rng.integers(0, 2, size=n, dtype=np.uint64)
    cts = rng.integers(0, 1 << 64, size=(count, n + 1), dtype=np.uint64)
    expected = rng.integers(0, 2 * p, size=count).astype(np.uint64)
    st, hst = api.NoiseStats(), api.NoiseStats()
    want = api.lwe_rotation_batch(s, cts, 1 << log_n, p, expected=expected, stats=hst, want=ALL)
    same_outputs(ctx.lwe_rotation_batch(s, cts, 1 << log_n, p, expected=expected, stats=st, want=ALL), want, ALL)
    assert st.as_dict() == hst.as_dict() and st.count == count and 0 < st.failures < count
    assert want["rot"][-1] == R.rotation(s, cts[-1], log_n) and st.std() == hst.std() and st.tail_log2(10) == hst.tail_log2(10)


def test_a_bad_key_word_on_the_device_is_refused_with_its_index(ctx):
    n = 70
    key = np.ones(n, np.uint64)
    key[66], key[68], key[3] = np.uint64(2), np.uint64(P - 1), np.uint64(P + 1)       # word 3 is 1 after reduction
    cts = np.zeros((9, n + 1), np.uint64)
    d_key, d_cts = to_dev(key), to_dev(cts)
    st = api.NoiseStats()
    with pytest.raises(api.VpbsError, match="key word 66 is neither 0 nor 1"):        # found by the kernel
        ctx.lwe_rotation_batch(d_key.data_ptr(), d_cts.data_ptr(), 128, 2, count=9, stats=st, n_lwe=n)
    assert st.count == 0
    with pytest.raises(api.VpbsError, match="key word 66 is neither 0 nor 1"):        # found before the launch
        ctx.lwe_rotation_batch(key, cts, 128, 2)
    key[66] = key[68] = np.uint64(0)
    assert ctx.lwe_rotation_batch(key, cts, 128, 2)["idx"].tolist() == [0] * 9         # the context stays usable


# ---- the prediction contract, at the shape of tests/test_gpu_multi_lut.py::test_messages_at_sigma_zero ----
LOG_N, K, ELL, LOGB, n5, p2 = 7, 2, 8, 8, 5, 2
TABLES = [[0, 1], [1, 0], [1, 1], [0, 0]]


@pytest.fixture(scope="module")
def noise_free():
    ring = T.Ring(LOG_N)
    rng = np.random.default_rng(5150)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n5, K, ELL, LOGB)
    words, cts = R.contract_rows(rng, s_lwe, LOG_N, p2)
    return dict(ring=ring, s_to=s_to, s_lwe=np.array(s_lwe, np.uint64), bsk_flat=np.stack([T.flatten_ggsw(g) for g in bsk]),
                ksk_flat=T.flatten_ggsw(ksk), words=words, cts=cts)


@pytest.mark.parametrize("theta", [0, 1, 2])
def test_the_bootstrap_reads_what_the_call_predicts(ctx, noise_free, theta):
    """125 noise-free ciphertexts whose phases step in quarter positions across every block edge (rotation_oracle.contract_rows), ELL * LOGB = 64:
    one Bootstrapper.run, and coefficient j of every output GLWE, and the extracted LWE, decrypt to lut_expect(testv, mu, j).  The rounded
    PHASE does not predict this: on some rows lwe_decode_batch's message under modulus 2p is another table position than idx (seed 5150:
    the restatement shows it on the CPU, asserted below).  theta 1, 2: the rows are snapped, the test vector packs 2^theta tables; mu from
    the snapped rows with log_slots 0 and from the raw rows with log_slots theta agree."""
    k = noise_free
    N, s = 1 << LOG_N, 1 << theta
    delta = T.get_delta(2 * p2)
    cts = k["cts"]
    assert len(cts) == 125 >= 64
    testv = api.lut_testv_multi(N, p2, np.array(TABLES[:s], np.uint64), delta)[0] if theta else api.lut_testv(N, p2, TABLES[1], delta)[0]
    rows = api.lwe_snap(N, theta, cts) if theta else cts
    got = ctx.lwe_rotation_batch(k["s_lwe"], rows, N, p2, want=ALL)
    raw = ctx.lwe_rotation_batch(k["s_lwe"], cts, N, p2, log_slots=theta, want=ALL)
    same_outputs(raw, got, ALL)
    mus, idxs, _ = R.rotation_batch(k["s_lwe"], cts, LOG_N, p2, theta)
    assert got["rot"].tolist() == mus and got["idx"].tolist() == idxs
    # the honest-test condition, from the restatement and from the device
    _, msgs, _ = O.decode_batch(k["s_lwe"], rows, delta, 2 * p2)
    assert sum(int(a != b) for a, b in zip(idxs, msgs)) >= 1
    dec = ctx.lwe_decode_batch(k["s_lwe"], rows, delta, 2 * p2, want=("msg",))["msg"]
    assert dec.tolist() == msgs and (got["idx"] != dec).sum() >= 1
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=125)
    out_ct, lwe_out = bs.run(rows, testv)
    bs.close()
    for r in range(125):
        mu = int(got["rot"][r])
        coeffs = T.glwe_decrypt(k["ring"], k["s_to"][:K - 1], B.glwe_list(out_ct[r]), K)
        for j in range(4):
            assert coeffs[j] == api.lut_expect(testv, mu, j), (r, j)
        assert B.lwe_decrypt(k["s_lwe"], lwe_out[r]) == api.lut_expect(testv, mu, 0), r


@pytest.mark.parametrize("theta", [1, 2])
def test_program_margins_of_a_two_level_run(ctx, noise_free, theta):
    """the two-level program of test_messages_at_sigma_zero under this module's keys: Program.margins of the run's gate_cts, from host
    arrays and from a device pointer, is the per-gate call; no idx fails against the messages the gates read, and |dev| stays within
    (n + 1) 2^(theta - 1), the n + 1 roundings of at most 2^(theta - 1) positions that test's docstring derives"""
    k = noise_free
    N, s = 1 << LOG_N, 1 << theta
    delta = T.get_delta(2 * p2)
    tables = TABLES[:s]
    rev = tables[::-1]
    testvs = np.stack([api.lut_testv_multi(N, p2, np.array(t, np.uint64), delta)[0] for t in (tables, rev)])
    msgs = [1, 0]
    rng = np.random.default_rng(77 + theta)
    inputs = np.array([T.lwe_encrypt(rng, [int(v) for v in k["s_lwe"]], delta * m % P) for m in msgs], np.uint64)
    first = lambda g: 2 + g * s
    gates = [([(0, 1)], 0, 0, theta, s), ([(1, 1)], 0, 1, theta, s), ([(first(0) + 1, 1)], 0, 0, theta, s), ([(first(1) + s - 2, 1)], 0, 1, theta, s)]
    expected = np.array([msgs[0], msgs[1], tables[1][msgs[0]], rev[s - 2][msgs[1]]], np.uint64)      # the message every gate reads
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=4)
    prog = api.Program(ctx, 2, gates, 2)
    level = prog.levels()[0]
    assert level.tolist() == [1, 1, 2, 2]
    _, gate_cts, _ = prog.run(bs, inputs, testvs)
    bs.close()
    d_cts = to_dev(gate_cts)
    host = prog.margins(ctx, k["s_lwe"], gate_cts, [p2, p2], expected=expected, N=N)
    dev = prog.margins(ctx, k["s_lwe"], d_cts.data_ptr(), [p2, p2], expected=expected, N=N)
    null = prog.margins(None, k["s_lwe"], gate_cts, [p2, p2], expected=expected, N=N)
    prog.close()
    for mu, idx, dv, stats in (host, dev, null):
        for g in range(4):
            one = ctx.lwe_rotation_batch(k["s_lwe"], gate_cts[g:g + 1], N, p2, expected=expected[g:g + 1], want=ALL)
            assert (int(mu[g]), int(idx[g]), int(dv[g])) == (int(one["rot"][0]), int(one["idx"][0]), int(one["dev"][0])), g
        assert idx.tolist() == expected.tolist()
        assert [st.count for st in stats] == [2, 2] and all(st.failures == 0 for st in stats)
        assert int(np.abs(dv).max()) <= (n5 + 1) * (1 << (theta - 1))
        for lv, st in enumerate(stats, start=1):
            per = api.NoiseStats()
            api.lwe_rotation_batch(k["s_lwe"], gate_cts[level == lv], N, p2, expected=expected[level == lv], stats=per, want=())
            assert st.as_dict() == per.as_dict()

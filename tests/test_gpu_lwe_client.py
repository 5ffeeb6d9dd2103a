"""GPU tests (-m gpu) of the batched client calls (vpbs_lwe_encrypt_batch, vpbs_lwe_decode_batch; csrc/lwe_client.hip).  Yardsticks: the same
calls with a null context (the host path, itself held to the seeded restatement and to vpbs_lwe_decrypt by tests/test_lwe_client_cpu.py)
and Python integers (tests/lwe_client_oracle.py).  Exact arithmetic: every comparison is word for word.  The shapes are the stride edges
of the kernels: a wave takes a row 64 words at a time, a workgroup four rows, the grid 2048 workgroups."""
import numpy as np
import pytest
import torch

import lwe_client_oracle as O
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)       # main.rs:29-30
N_LWE = [1, 63, 64, 65, 255, 256, 257, 728]
COUNTS = [1, 2, 257]


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


def edge_key(rng, n, binary):
    """zero, one and non-binary words, one of them at or above p"""
    s = rng.integers(0, 2, size=n, dtype=np.uint64) if binary else rng.integers(0, P, size=n, dtype=np.uint64)
    s[n - 1] = np.uint64(P + 2)
    if n >= 4:
        s[0], s[1], s[2] = np.uint64(0), np.uint64(1), np.uint64(0x123456789ABCDEF)
    return s


@pytest.mark.parametrize("n_lwe", N_LWE)
def test_encrypt_on_the_device_is_the_host_call(ctx, n_lwe):
    rng = np.random.default_rng(1000 + n_lwe)
    prm = api.KeygenParamsC(10, 2, 4, 5, n_lwe, 0xABCD00 + n_lwe, *SIGMAS)
    s = edge_key(rng, n_lwe, binary=True)
    d_s = to_dev(s)
    delta = T.get_delta(4)
    for count in COUNTS:
        msgs = (rng.integers(0, 4, size=count, dtype=np.uint64) * np.uint64(delta))
        msgs[:3] = np.array([P - 1, 1, 0], np.uint64)[:count]
        nonce0 = (1 << 24) - count if count == 2 else 7 * count
        want = api.lwe_encrypt_batch(prm, s, msgs, nonce0=nonce0)
        got = ctx.lwe_encrypt_batch(prm, s, msgs, nonce0=nonce0)                              # host key, host output
        assert got.shape == want.shape and (got == want).all(), (count, np.argwhere(got != want)[:4].tolist())
        d_out = dev_zeros(count, n_lwe + 1)
        assert ctx.lwe_encrypt_batch(prm, d_s.data_ptr(), msgs, nonce0=nonce0, out_dev_ptr=d_out.data_ptr()) is None
        assert (back(d_out) == want).all(), count                                              # device key, device output
        if count == 257:
            assert (ctx.lwe_encrypt_batch(prm, d_s.data_ptr(), msgs, nonce0=nonce0) == want).all()          # device key, host output
            d_out2, d_m = dev_zeros(count, n_lwe + 1), to_dev(msgs)
            ctx.lwe_encrypt_batch(prm, s, d_m.data_ptr(), nonce0=nonce0, out_dev_ptr=d_out2.data_ptr(), count=count)   # host key, all else device
            assert (back(d_out2) == want).all()


def test_encrypt_refusals_on_the_device(ctx):
    prm = api.KeygenParamsC(10, 2, 4, 5, 70, 5, *SIGMAS)
    s = np.ones(70, np.uint64)
    msgs = np.array([0, 1, 2, P, 4, P + 1], np.uint64)
    with pytest.raises(api.VpbsError, match="message 3 is not below p"):
        ctx.lwe_encrypt_batch(prm, s, msgs)
    d_out, d_m = dev_zeros(6, 71), to_dev(msgs)
    with pytest.raises(api.VpbsError, match="message 3 is not below p"):                      # found by the kernel
        ctx.lwe_encrypt_batch(prm, s, d_m.data_ptr(), out_dev_ptr=d_out.data_ptr(), count=6)
    with pytest.raises(api.VpbsError, match="ciphertext 1 is the first without a nonce"):
        ctx.lwe_encrypt_batch(prm, s, msgs[:3], nonce0=(1 << 24) - 1)
    assert (ctx.lwe_encrypt_batch(prm, s, msgs[:3]) == api.lwe_encrypt_batch(prm, s, msgs[:3])).all()     # the context stays usable


def decode_case(rng, n, count, delta, modulus):
    """random rows with words at or above p under a non-binary key; the leading rows carry the half-way phases and the +-1, +-delta / 2 errors"""
    s = edge_key(rng, n, binary=False)
    cts = rng.integers(0, P, size=(count, n + 1), dtype=np.uint64)
    cts[0, 0] = np.uint64(P)
    cts[count - 1, n // 2] = np.uint64((1 << 64) - 1)
    edges = O.edge_phases(delta, modulus)[:max(count - 1, 0)]
    for i, target in enumerate(edges, start=1 if count > 1 else 0):
        cts[i, n] = 0
        cts[i, n] = np.uint64((target - O.phase(s, cts[i])) % P)
    if count > len(edges) + 2:
        cts[count - 2, n] = np.uint64(P + 5)                       # a body at or above p
    return s, cts, edges


def same_outputs(got, want, names):
    assert sorted(got) == sorted(names)
    for k in names:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), (k, np.argwhere(got[k] != want[k])[:4].tolist())


@pytest.mark.parametrize("n_lwe", N_LWE)
def test_decode_on_the_device_is_the_host_path_and_the_oracle(ctx, n_lwe):
    rng = np.random.default_rng(2000 + n_lwe)
    delta, modulus = T.get_delta(4), 4
    ALL = ("phase", "msg", "err")
    for count in COUNTS:
        s, cts, edges = decode_case(rng, n_lwe, count, delta, modulus)
        ost = O.Stats()
        ph, ms, er = O.decode_batch(s, cts, delta, modulus, None, ost)
        if count > 1:
            assert ph[1:1 + len(edges)] == edges                   # the rows do carry the phases they were built for
        expected = np.array(ms, np.uint64)
        expected[::5] = (expected[::5] + np.uint64(1)) % np.uint64(modulus)        # failures, among them row 0
        expected[count - 1] += np.uint64(modulus)                   # equal mod modulus: no failure, but err is measured from it
        ost_e = O.Stats()
        ph_e, ms_e, er_e = O.decode_batch(s, cts, delta, modulus, expected, ost_e)
        d_cts, d_s, d_exp = to_dev(cts), to_dev(s), to_dev(expected)
        for exp, d_e, o_stats, o_err in ((None, None, ost, er), (expected, d_exp, ost_e, er_e)):
            hst, st0, st2, st1 = api.NoiseStats(), api.NoiseStats(), api.NoiseStats(), api.NoiseStats()
            want = api.lwe_decode_batch(s, cts, delta, modulus, expected=exp, stats=hst, want=ALL)                  # null context
            assert want["phase"].tolist() == ph and want["msg"].tolist() == ms and want["err"].tolist() == o_err
            assert hst.as_dict() == o_stats.as_dict()
            same_outputs(ctx.lwe_decode_batch(s, cts, delta, modulus, expected=exp, stats=st0, want=ALL), want, ALL)   # host pointers
            got = ctx.lwe_decode_batch(d_s.data_ptr(), d_cts.data_ptr(), delta, modulus, expected=None if exp is None else d_e.data_ptr(),
                                       count=count, stats=st2, want=ALL, n_lwe=n_lwe)                                # outputs to the host
            same_outputs(got, want, ALL)
            d_o = {k: dev_zeros(count) for k in ALL}
            assert ctx.lwe_decode_batch(s, d_cts.data_ptr(), delta, modulus, expected=exp, count=count, stats=st1,
                                        want={k: d.data_ptr() for k, d in d_o.items()}) is None                       # all on the device
            for k in ALL:
                assert (back(d_o[k]) == want[k].view(np.uint64)).all(), k
            for st in (st0, st2, st1):
                assert st.as_dict() == o_stats.as_dict()
                assert st.failures == (0 if exp is None else len(range(0, count, 5)))
            # each output pointer NULL in turn, and no statistics
            for drop in ALL:
                names = tuple(k for k in ALL if k != drop)
                same_outputs(ctx.lwe_decode_batch(s, d_cts.data_ptr(), delta, modulus, expected=exp, count=count, want=names), want, names)
        if count == 257:
            # three launches into one struct are one pass of the oracle; the middle one starts in the middle of a workgroup's four rows
            st = api.NoiseStats()
            for lo, hi in ((0, 101), (101, 200), (200, 257)):
                ctx.lwe_decode_batch(d_s.data_ptr(), d_cts.data_ptr() + 8 * lo * (n_lwe + 1), delta, modulus, expected=expected[lo:hi],
                                     count=hi - lo, stats=st, want=(), n_lwe=n_lwe)
            assert st.as_dict() == ost_e.as_dict() and st.count == 257


def test_decode_statistics_past_64_and_128_bits_and_a_full_grid(ctx):
    """errors near p / 2 under delta = p (the sums pass 128 bits after a few rows) in a batch of more rows than the grid has waves
    (2048 workgroups of four): every wave walks more than one row"""
    n, count = 3, 4 * 2048 * 2 + 37
    rng = np.random.default_rng(9)
    phases = rng.integers((P - 1) // 2 - 1000, (P - 1) // 2 + 1000, size=count, dtype=np.uint64)
    cts = np.zeros((count, n + 1), np.uint64)
    cts[:, n] = phases
    s = np.zeros(n, np.uint64)
    want = O.Stats()
    _, _, er = O.decode_batch(s, cts, P, 1, None, want)
    st, hst = api.NoiseStats(), api.NoiseStats()
    got = ctx.lwe_decode_batch(s, cts, P, 1, stats=st, want=("err",))
    assert got["err"].tolist() == er and st.as_dict() == want.as_dict() and st.sum_sq >> 128
    api.lwe_decode_batch(s, cts, P, 1, stats=hst, want=())
    assert hst.as_dict() == want.as_dict()
    assert st.std() == hst.std() and st.mean() == hst.mean()


# ---- closing the loop at the small ring of tests/test_gpu_program.py: encrypt on the device -> Program.run_device -> decode on the device ----
LOG_N, K, ELL, LOGB, n5 = 6, 2, 8, 8, 5
TABLES = [[0, 1], [1, 0]]                    # p = 2: messages live mod 2 p = 4; a gate input in [2, 4) yields the negated entry
one = lambda w, lut: ([(w, 1)], 0, lut)
add = lambda a, b, lut, const=0: ([(a, 1), (b, 1)], const, lut)
DELTA = T.get_delta(4)
# 3 inputs (wires 0 1 2), 7 gates (wires 3 .. 9), levels 1 1 1 2 2 3 3
LOOP = [one(0, 0), add(1, 2, 1), add(0, 2, 0),                   # 1;  NOT(0 + 1) = 0;  1 + 1 = 2 -> -T0[0] = 0 (an XOR)
        add(3, 4, 1), ([(3, 2)], 0, 1),                          # NOT(1 + 0) = 0;  2 * 1 = 2 -> -T1[0] = -1 = 3
        one(7, 0), add(6, 5, 1, const=DELTA)]                    # 3 -> -T0[1] = 3;  NOT(0 + 0 + 1) = 0
LOOP_MSGS = [1, 0, 1]


def plain_evaluation(msgs, gates, tables, p, delta):
    w = list(msgs)
    for terms, const, lut in gates:
        c = (const // delta + sum(coef * w[src] for src, coef in terms)) % (2 * p)
        w.append(tables[lut][c] % (2 * p) if c < p else -tables[lut][c - p] % (2 * p))
    return w


@pytest.mark.parametrize("sigmas", [(0.0, 0.0), SIGMAS])
def test_the_loop_closes_on_the_device(ctx, sigmas):
    """Seed 0x10CA1 was chosen on the CPU: with these keys (tfhe_oracle.seeded_pbs_keys), inputs (seeded_lwe_encrypt) and tables, the reference
    arithmetic of tests/tfhe_oracle.py (pbs_chain per gate, partial sample extraction, combination in Python integers) decodes every wire
    of LOOP to its plain value, at sigma 0 (every err is 0) and at the paper's sigmas (largest |err| = 0.166 delta, against the delta / 2
    at which a message decodes wrongly)."""
    N, seed = 1 << LOG_N, 0x10CA1
    want = plain_evaluation(LOOP_MSGS, LOOP, TABLES, 2, DELTA)
    assert want == [1, 0, 1, 1, 0, 0, 0, 3, 3, 0]
    keys = ctx.keygen_device(N, K, ELL, LOGB, n5, seed, *sigmas)
    d_key = ctx.device_upload_new(keys["s_lwe"])
    testvs = np.stack([api.lut_testv(N, 2, t)[0] for t in TABLES])
    assert (testvs[0] == api.testv(N, 2)[0]).all()
    d_tv, d_in, d_w = to_dev(testvs), dev_zeros(3, n5 + 1), dev_zeros(10, n5 + 1)
    ctx.lwe_encrypt_batch(keys["params"], d_key, [DELTA * m for m in LOOP_MSGS], nonce0=50, out_dev_ptr=d_in.data_ptr())   # born on the device
    bs = api.Bootstrapper(ctx, keys["d_bsk"], keys["d_ksk"], K, ELL, LOGB, max_batch=2, N=N, n_lwe=n5, keys_on_device=True)
    prog = api.Program(ctx, 3, LOOP, 2)
    assert prog.levels()[0].tolist() == [1, 1, 1, 2, 2, 3, 3]
    assert prog.run_device(bs, d_in.data_ptr(), d_tv.data_ptr(), d_w.data_ptr()) == 3
    st = api.NoiseStats()
    got = ctx.lwe_decode_batch(d_key, d_w.data_ptr(), DELTA, 4, expected=want, count=10, stats=st, want=("msg", "err"), n_lwe=n5)
    assert got["msg"].tolist() == want and st.failures == 0 and st.count == 10
    assert st.max_abs < DELTA // 2 and st.max_abs == int(np.abs(got["err"]).max())
    if sigmas == (0.0, 0.0):
        assert got["err"][:3].tolist() == [0, 0, 0]              # the inputs carry no noise
    # the host path on the downloaded wires says the same
    hst = api.NoiseStats()
    host = api.lwe_decode_batch(keys["s_lwe"], back(d_w), DELTA, 4, expected=want, stats=hst, want=("msg", "err"))
    assert (host["msg"] == got["msg"]).all() and (host["err"] == got["err"]).all() and hst.as_dict() == st.as_dict()
    # one deliberately wrong expectation: one failure, and that index's message is unchanged
    wrong = list(want)
    wrong[6] = (wrong[6] + 1) % 4
    st2 = api.NoiseStats()
    got2 = ctx.lwe_decode_batch(d_key, d_w.data_ptr(), DELTA, 4, expected=wrong, count=10, stats=st2, want=("msg",), n_lwe=n5)
    assert st2.failures == 1 and st2.count == 10 and got2["msg"].tolist() == want
    prog.close()
    bs.close()
    for d in (d_key, keys["d_bsk"], keys["d_ksk"]):
        ctx.device_free(d)

"""GPU tests (-m gpu): where the library's streams come from (csrc/api.hip, DESIGN.md 5 Host side).  A context creates its prover stream and
nothing else; the host->device copies of vpbs_device_upload_bg go through ONE stream per device, made by the first upload of any context there,
shared by all of them and destroyed with the last context.  vpbs_test_stream_counts reports (prover streams, auxiliary streams) of a device.
The counts are checked against the counts at each test's entry."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

import vpbs_amd
from vpbs_amd import api, synth

pytestmark = pytest.mark.gpu
SIZES = (1, 4099, 65536)          # words: one, an odd count past a page, a power of two
TAIL = 8                          # sentinel words behind every device buffer


def counts(device=0):
    out = (C.c_uint * 2)()
    assert api.lib().vpbs_test_stream_counts(device, out) == 0
    return out[0], out[1]


class Held:
    """the counts at a test's entry; `holds(provers, aux)`: this test's contexts have added exactly `provers` prover streams, and -- where the
    library held nothing at entry, the ordinary case -- exactly `aux` auxiliary ones.  A context another test left open (a traceback that keeps
    it alive, a fixture of wider scope) may own the device's upload stream already: then the count may only stay or grow by that one stream"""

    def __init__(self):
        gc.collect()
        self.base = counts()

    def holds(self, provers, aux):
        got = counts()
        assert got[0] == self.base[0] + provers, (got, self.base)
        if self.base == (0, 0):
            assert got[1] == aux, (got, self.base)
        else:
            assert self.base[1] <= got[1] <= self.base[1] + 1, (got, self.base)
        return True


@pytest.fixture
def held():
    h = Held()
    yield h
    gc.collect()
    assert h.holds(0, 0), "the test left a stream behind"


def pattern(thread, rnd, words):
    return (np.uint64(thread + 1) << np.uint64(56)) + (np.uint64(rnd + 1) << np.uint64(48)) + (np.uint64(words) << np.uint64(24)) + \
        np.arange(words, dtype=np.uint64)


def pinned(words):
    import torch
    return torch.empty(words, dtype=torch.int64).pin_memory()


def device_buffer(words):
    import torch
    return torch.full((words + TAIL,), -1, dtype=torch.int64, device="cuda")


def upload_and_check(c, seed, words=4099):
    """one upload through `c`, read back word for word"""
    import torch
    host, dev = pinned(words), device_buffer(words)
    host.numpy().view(np.uint64)[:] = pattern(seed, 0, words)
    torch.cuda.synchronize()       # the fill ran on torch's stream, the copy runs on the library's
    c.upload_bg(dev.data_ptr(), host.data_ptr(), words)
    got = dev.cpu().numpy().view(np.uint64)
    assert (got[:words] == pattern(seed, 0, words)).all() and (got[words:] == np.uint64(2**64 - 1)).all()


def test_concurrent_uploads_through_the_shared_stream(held):
    """four contexts, four uploading threads (own patterns of 1, 4 099 and 65 536 words, three rounds) while a step proof of degree 2^5 runs
    on every context's stream: every buffer holds exactly its pattern, nothing behind it is touched, and the proofs are what they were"""
    import torch
    n_ctx, rounds, log_n = 4, 3, 5
    ctxs = [vpbs_amd.Context(0, log_n_max=10) for _ in range(n_ctx)]
    inputs = synth.step_inputs(log_n)
    digest, pis = np.array([1, 2, 3, 4], np.uint64), synth.field_elements(9, 8)
    css = [c.commit_values(inputs["constants_sigmas"]) for c in ctxs]
    sis = [c.make_step_inputs(log_n, inputs["wires"], inputs["zs_partial_products"], inputs["quotient"], cs, digest, pis)
           for c, cs in zip(ctxs, css)]
    want = ctxs[0].prove_step(sis[0])
    hosts = {(t, r, w): pinned(w) for t in range(n_ctx) for r in range(rounds) for w in SIZES}
    devs = {key: device_buffer(key[2]) for key in hosts}
    for (t, r, w), h in hosts.items():
        h.numpy().view(np.uint64)[:] = pattern(t, r, w)
    torch.cuda.synchronize()
    assert held.holds(n_ctx, 0)
    errors, uploading = [], threading.Event()
    start = threading.Barrier(2 * n_ctx)

    def uploader(t):
        try:
            start.wait()
            for r in range(rounds):
                for w in SIZES:
                    ctxs[t].upload_bg(devs[t, r, w].data_ptr(), hosts[t, r, w].data_ptr(), w)
        except Exception as e:                                                        # noqa: BLE001
            errors.append(e)

    def prover(t):
        try:
            start.wait()
            while True:
                p = ctxs[t].prove_step(sis[t])
                assert all((p[k] == want[k]).all() for k in ("caps", "openings", "fri"))
                if uploading.is_set():
                    return
        except BaseException as e:                                                    # noqa: BLE001
            errors.append(e)

    ups = [threading.Thread(target=uploader, args=(t,)) for t in range(n_ctx)]
    prs = [threading.Thread(target=prover, args=(t,)) for t in range(n_ctx)]
    for th in ups + prs:
        th.start()
    for th in ups:
        th.join()
    uploading.set()
    for th in prs:
        th.join()
    assert not errors, errors
    assert held.holds(n_ctx, 1)
    for (t, r, w), d in devs.items():
        got = d.cpu().numpy().view(np.uint64)
        assert (got[:w] == pattern(t, r, w)).all(), (t, r, w)
        assert (got[w:] == np.uint64(2**64 - 1)).all(), (t, r, w)
    for c, cs in zip(ctxs, css):
        cs.free()
        c.close()


def test_eight_contexts_hold_eight_prover_streams_and_one_upload_stream(held):
    ctxs = [vpbs_amd.Context(0, log_n_max=10) for _ in range(8)]
    assert held.holds(8, 0)
    upload_and_check(ctxs[3], 3)
    assert held.holds(8, 1)
    for i, c in enumerate(ctxs):
        upload_and_check(c, i)
    assert held.holds(8, 1)
    for c in ctxs:
        c.close()


def test_the_shared_stream_lives_as_long_as_any_context(held):
    a, b = vpbs_amd.Context(0, log_n_max=10), vpbs_amd.Context(0, log_n_max=10)
    upload_and_check(a, 1)
    assert held.holds(2, 1)
    a.close()                                   # the context that made the stream goes; the stream is b's as well
    assert held.holds(1, 1)
    upload_and_check(b, 2)
    b.synchronize()
    b.close()
    assert held.holds(0, 0)
    c = vpbs_amd.Context(0, log_n_max=10)
    assert held.holds(1, 0)
    upload_and_check(c, 3)
    assert held.holds(1, 1)
    c.close()


def test_contexts_that_never_upload_add_no_stream(held):
    """a context that only proves, and the two witness contexts of a chain's device pipeline (a whole n = 1 chain runs through them)"""
    import export_circuits
    import tfhe_oracle as T
    from test_cyclic_cpu import n8_chain_inputs
    from vpbs_amd import circuit_file
    N, K, ELL, LOGB, LOG_N = 8, 2, 4, 5, 13
    c = vpbs_amd.Context(0, log_n_max=16)
    inputs = synth.step_inputs(5)
    cs = c.commit_values(inputs["constants_sigmas"])
    si = c.make_step_inputs(5, inputs["wires"], inputs["zs_partial_products"], inputs["quotient"], cs, np.array([1, 2, 3, 4], np.uint64),
                            synth.field_elements(9, 8))
    c.prove_step(si)
    cs.free()
    assert held.holds(1, 0)
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, 1, LOG_N)]
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    ivc.set_device_witness(ELL, LOGB, 2, False)
    assert held.holds(3, 0)
    ivc.prove_pbs(testv, ct, np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk))
    assert held.holds(3, 0)
    ivc.set_device_witness(ELL, LOGB, 0)
    assert held.holds(1, 0)
    ivc.free()
    c.close()

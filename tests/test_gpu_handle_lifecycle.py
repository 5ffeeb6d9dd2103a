"""GPU test (-m gpu) of the one order of closing that the context's registry makes legal for every wrapper of a C handle (api._Handle):
the Context first, its objects afterwards.  Each object runs once and is compared with its own suite's yardstick, so that what is closed
has really been used; then a second Context shows the device was left usable."""
import numpy as np
import pytest

import oracle as orc
import vpbs_amd
from test_gpu_pbs_batch import SIGMAS
from test_gpu_witness_check import step_circuit_n8
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
N, K, ELL, LOGB, n = 64, 3, 3, 7, 40


def bootstrap_and_check(ctx, keys, cts, tv):
    """a Bootstrapper on the context, one run, every accumulator against the per-step path (test_gpu_pbs_batch's yardstick) -> (object, outputs)"""
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=len(cts))
    out_ct, lwe_out, accs = bs.run(cts, tv, accumulators=True)
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), tv.reshape(1, N)])
    for i in range(len(cts)):
        want = ctx.pbs_accumulator_chain(acc_init, cts[i], keys["bsk"], keys["ksk"], K, ELL, LOGB)
        assert (accs[i] == want).all() and (out_ct[i] == want[-1]).all(), i
        assert (lwe_out[i] == ctx.lwe_extract(want[-1], n)).all(), i
    return bs, (out_ct, lwe_out)


def test_the_context_may_be_closed_before_its_objects():
    ctx = vpbs_amd.Context(0, log_n_max=16)
    vals = np.random.default_rng(5).integers(0, P, size=(2, 1 << 5), dtype=np.uint64)
    batch = ctx.commit_values(vals)
    assert (batch.cap() == orc.Batch(vals, 3, 4, True).cap()).all()
    keys = ctx.keygen(N, K, ELL, LOGB, n, 0x777, *SIGMAS)
    tv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(2)])
    bs, want = bootstrap_and_check(ctx, keys, cts, tv)
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=2, max_batch=2)
    assert ring.add(keys["bsk"], keys["ksk"]) == 0
    got = ring.run(cts, [0, 0], tv)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    circ, b, plan, _, w = step_circuit_n8()
    h = api.hash_no_pad(np.array(circ.public_inputs(w), np.uint64))
    chk = api.WitnessChecker(ctx, b.circuit)
    assert chk.check(w, h) == b.circuit.check_witness(w, h) == (True, "")
    objs = [batch, bs, ring, chk]
    assert all(o in ctx._batches for o in objs)
    ctx.close()
    assert ctx.h is None and all(o.h is None for o in objs)
    for o in objs:   # nothing is left to free: no call reaches the library
        o.close()
        o.free()
        assert o.h is None
    plan.free()
    ctx.close()
    ctx2 = vpbs_amd.Context(0, log_n_max=16)   # the device is as usable as before
    bs2, again = bootstrap_and_check(ctx2, keys, cts, tv)
    assert (again[0] == want[0]).all() and (again[1] == want[1]).all()
    bs2.close()
    ctx2.close()

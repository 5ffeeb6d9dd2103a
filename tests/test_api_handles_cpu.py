"""The Python objects that wrap a C handle share one lifecycle (api._Handle): checked here on a recording stand-in for the library -- no
device and no library call -- for EVERY subclass, found by walking _Handle.__subclasses__(), so that a class added later is covered as it
is.  And the ctypes table api.SIGNATURES against the header, for all symbols: return type and arity."""
import ctypes as C
import os
import sys
import types
import weakref

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeLib:
    """every vpbs_*_free, and vpbs_ctx_destroy, appends (name, handle) to .calls; nothing else exists"""

    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def __getattr__(self, name):
        if not (name.endswith("_free") or name == "vpbs_ctx_destroy"):
            raise AttributeError(name)

        def record(h):
            self.calls.append((name, h))
            if self.fail:
                raise RuntimeError("free failed")
        return record


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(api, "_lib", f)
    return f


def handle_classes():
    found, stack = [], list(api._Handle.__subclasses__())
    while stack:
        cls = stack.pop()
        stack += cls.__subclasses__()
        if cls._prefix is not None:   # _BatchProver, _ChainRun, _PbsVerify: shared bodies without a C object of their own
            found.append(cls)
    return sorted(set(found), key=lambda c: c.__name__)


CLASSES = handle_classes()


def stub_context():
    return types.SimpleNamespace(h=1, _batches=weakref.WeakSet())


def make(cls, ctx, h=0x1234):
    obj = cls.__new__(cls)
    obj.h = h
    obj._created(ctx)
    return obj


def test_every_wrapper_is_found():
    names = {c.__name__ for c in CLASSES}
    assert {"WitnessPlan", "WitnessChecker", "WitnessDevice", "ProofVerifier", "Ivc", "PbsVerifier", "Bootstrapper", "KeyRing", "PbsProver",
            "RingProver", "RingVerifier", "Aggregator", "AggregateVerifier", "Program", "Batch"} <= names
    for cls in CLASSES:   # one lifecycle: nobody writes a close, a free or a finalizer of its own
        for name in ("close", "free", "__del__"):
            assert getattr(cls, name) is getattr(api._Handle, name), (cls.__name__, name)
        assert (cls._prefix + "_free") in api.SIGNATURES, cls.__name__


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_close_frees_once_and_leaves_the_registry(fake, cls):
    ctx = stub_context()
    obj = make(cls, ctx)
    assert obj in ctx._batches
    obj.close()
    assert fake.calls == [(cls._prefix + "_free", 0x1234)]
    assert obj.h is None and obj not in ctx._batches
    obj.close()
    obj.free()
    obj.__del__()
    assert len(fake.calls) == 1


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_a_failing_free_does_not_leave_the_finalizer(monkeypatch, cls):
    f = FakeLib(fail=True)
    monkeypatch.setattr(api, "_lib", f)
    ctx = stub_context()
    obj = make(cls, ctx)
    obj.__del__()   # must not raise
    assert len(f.calls) == 1 and obj.h is None and obj not in ctx._batches
    with pytest.raises(RuntimeError):   # close itself reports it
        make(cls, ctx).close()


def test_an_object_without_a_context(fake):
    for cls in (api.WitnessPlan, api.PbsProver, api.Program):
        obj = make(cls, None, h=5)
        assert obj.ctx is None
        obj.close()
        obj.close()
    assert [c[1] for c in fake.calls] == [5, 5, 5]


def test_context_close_frees_the_survivors_then_itself(fake):
    ctx = api.Context.__new__(api.Context)
    ctx.h, ctx._batches = 7, weakref.WeakSet()
    objs = [make(api.WitnessDevice, ctx, 21), make(api.Ivc, ctx, 22), make(api.WitnessChecker, ctx, 23), make(api.Batch, ctx, 24)]
    gone = make(api.Bootstrapper, ctx, 25)
    gone.close()
    del fake.calls[:]
    ctx.close()
    assert sorted(fake.calls[:-1]) == [("vpbs_batch_free", 24), ("vpbs_ivc_free", 22), ("vpbs_witness_checker_free", 23),
                                      ("vpbs_witness_device_free", 21)]
    assert fake.calls[-1] == ("vpbs_ctx_destroy", 7) and ctx.h is None
    assert all(o.h is None for o in objs) and len(ctx._batches) == 0
    for o in objs + [gone]:   # the order the registry makes legal: the context first, the objects afterwards
        o.close()
        o.free()
    ctx.close()
    assert len(fake.calls) == 5


def test_a_batch_whose_context_is_gone_is_only_forgotten(fake):
    ctx = stub_context()
    b = make(api.Batch, ctx, 31)
    ctx.h = None
    b.free()
    assert fake.calls == [] and b.h is None and b not in ctx._batches


def test_the_ring_provers_view_is_never_freed(fake):
    ring_ctx = api._RingContext(3)
    view = api.KeyRing._view(12, ring_ctx, 8, 2, 2, 4, 6, 3, 256)
    assert isinstance(view, api.KeyRing) and (view.N, view.K, view.ELL, view.LOGB, view.n_lwe, view.max_keys, view.max_batch) == (8, 2, 2, 4, 6, 3, 256)
    assert view not in ring_ctx._batches
    view.close()
    view.free()
    assert fake.calls == [] and view.h is None
    rp = api.RingProver.__new__(api.RingProver)
    rp.h, rp.keyring = 11, api.KeyRing._view(12, ring_ctx, 8, 2, 2, 4, 6, 3, 256)
    rp.close()
    assert fake.calls == [("vpbs_ring_prover_free", 11)] and rp.h is None and rp.keyring.h is None   # the view goes with the prover
    rp.close()
    rp.keyring.close()
    rp.keyring.__del__()
    assert len(fake.calls) == 1
    owned = make(api.KeyRing, stub_context(), 13)   # a ring of its own is freed
    owned.close()
    assert fake.calls[-1] == ("vpbs_keyring_free", 13)


def test_status_errors():
    e = api.VpbsError("x", status=-3)
    assert str(e) == "x" and e.status == -3 and not hasattr(api.VpbsError("x"), "status")
    assert api.WitnessError("w").status == api.ERR_WITNESS
    f = api._Handle._fail
    assert str(f("vpbs_x_run", -2, "why")) == "vpbs_x_run: status -2: why" and f("vpbs_x_run", -2, "why").status == -2
    assert str(f("vpbs_x_run", -2)) == "vpbs_x_run: status -2" and str(f("vpbs_x_run", -2, "")) == "vpbs_x_run: status -2: "
    assert str(f("", -1, "text")) == "status -1: text"


def test_the_pointer_vocabulary():
    a = np.arange(3, dtype=np.uint64)
    assert api._keep_ptr(None) is None and api._keep_u32(None) is None and api._dev(None) is None and api._dev(0) is None
    assert api._keep_ptr(a)[2] == 2 and C.addressof(api._keep_ptr(a).contents) == a.ctypes.data
    assert api._keep_ptr(np.zeros((0, 4), np.uint64))[0] == 0          # an empty array still gives a pointer that can be read
    assert api._keep_u32(np.zeros(0, np.uint32))[0] == 0 and api._keep_u32(np.array([7], np.uint32))[0] == 7
    assert api._dev(4096).value == 4096 and api._dev(np.uint64(4096)).value == 4096
    for bad in (np.zeros(2, np.uint32), np.zeros((4, 4), np.uint64)[:, ::2]):
        with pytest.raises(AssertionError):
            api._keep_ptr(bad)
    with pytest.raises(AssertionError):
        api._keep_u32(np.zeros(2, np.uint64))


def test_packing():
    blobs = [b"abc", b"", b"defgh"]
    count, data, offs, outs, ptrs = api._packed(blobs, outputs=2)
    assert count == 3 and [offs[i] for i in range(4)] == [0, 3, 3, 8] and bytes(data[:8]) == b"abcdefgh"
    assert len(outs) == len(ptrs) == 2 and all(o.shape == (3,) and o.dtype == np.uint8 and not o.any() for o in outs)
    assert all(C.addressof(p.contents) == o.ctypes.data for p, o in zip(ptrs, outs))
    buf, offsets = api.pack_proofs(blobs)
    count, data, offs, outs, ptrs = api._packed(buf, offsets, shape=(1, 3), outputs=3)
    assert count == 3 and bytes(data[:8]) == b"abcdefgh" and [o.shape for o in outs] == [(1, 3)] * 3
    count, data, offs, outs, ptrs = api._packed([])                      # no proofs: pointers all the same
    assert count == 0 and offs[0] == 0 and data[0] == 0 and outs == () and ptrs == []
    assert api._packed(np.zeros(0, np.uint8), np.zeros(0, np.uint64), outputs=1)[3][0].shape == (0,)   # no offsets at all: count -1, empty results


def test_shape_and_key_helpers():
    N, K, ELL, n = 8, 2, 2, 3
    g = K * ELL * K * N
    c, tv = api._cts_testv("X.run", N, n, np.zeros((2, n + 1)), np.zeros(N))
    assert c.dtype == tv.dtype == np.uint64 and c.shape == (2, n + 1)
    assert api._cts_testv("X.run", N, n, np.zeros((0, n + 1)), np.zeros((0, N)))[0].shape == (0, n + 1)
    for cts, testv in ((np.zeros((2, n)), np.zeros(N)), (np.zeros(n + 1), np.zeros(N)), (np.zeros((2, n + 1)), np.zeros((3, N)))):
        with pytest.raises(ValueError, match=r"X\.run: expected cts \[count\]\[4\] and testv \[8\] or \[count\]\[8\]"):
            api._cts_testv("X.run", N, n, cts, testv)
    bsk, ksk = np.ones((n, g), np.uint64), np.ones(g, np.uint64)
    pb, pk, N_, n_, keep = api._key_args("Bootstrapper", bsk, ksk, K, ELL, None, None, False)     # the shape is read off the arrays
    assert (N_, n_) == (N, n) and pb.value == keep[0].ctypes.data and pk.value == keep[1].ctypes.data
    assert api._key_args("KeyRing.add", bsk, ksk, K, ELL, N, n, False)[2:4] == (N, n)
    with pytest.raises(ValueError, match=r"Bootstrapper: expected bsk \[n\]\[K\*ELL\*K\*N\] and ksk \[K\*ELL\*K\*N\]"):
        api._key_args("Bootstrapper", bsk[:, :-1], ksk, K, ELL, None, None, False)
    with pytest.raises(ValueError, match=r"KeyRing\.add: expected bsk \[4\]\[%d\] and ksk \[%d\]" % (g, g)):
        api._key_args("KeyRing.add", bsk, ksk, K, ELL, N, n + 1, False)
    with pytest.raises(ValueError, match="PbsProver: device keys need N and n_lwe"):
        api._key_args("PbsProver", 4096, 8192, K, ELL, None, n, True)
    pb, pk, N_, n_, keep = api._key_args("RingProver.add", 4096, 8192, K, ELL, N, n, True)
    assert (pb.value, pk.value, N_, n_, keep) == (4096, 8192, N, n, None)


def test_signatures_have_the_headers_return_type_and_arity():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    functions = gen_rust_ffi.Binding(open(gen_rust_ffi.HEADER).read()).functions
    scalars = {None: None, "i32": C.c_int, "u32": C.c_uint, "u64": C.c_uint64, "c_long": C.c_long, "usize": C.c_size_t}

    def restype(rust):
        if rust in scalars:
            return scalars[rust]
        assert rust.startswith("*"), rust   # a return type the table has no word for yet: teach this test
        return C.c_char_p if rust.endswith("c_char") else C.c_void_p
    assert len(functions) >= 200 and {f[0] for f in functions} == set(api.SIGNATURES)
    for name, params, ret in functions:
        res, args = api.SIGNATURES[name]
        assert res is restype(ret), (name, res, ret)
        assert len(args) == len(params), (name, len(args), len(params))


class TypedFake:
    """every entry of api.SIGNATURES: checks the arity and converts each argument with the table's argtype, as ctypes does before a
    call; returns what .ret holds for the entry (0 unless set)"""

    def __init__(self):
        self.calls, self.ret = [], {"vpbs_last_error": b"boom"}

    def __getattr__(self, name):
        if name not in api.SIGNATURES:
            raise AttributeError(name)
        argtypes = api.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            for i, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except Exception as e:
                    raise AssertionError("%s: argument %d, %r, is no %s: %s" % (name, i, a, t.__name__, e))
            self.calls.append(name)
            return self.ret.get(name, 0)
        return call


N, K, ELL, LOGB, N_LWE = 8, 2, 2, 4, 3


SHAPED = []


@pytest.fixture
def typed(monkeypatch):
    f = TypedFake()
    monkeypatch.setattr(api, "_lib", f)
    yield f
    for obj in SHAPED:   # their handles are made up: no finalizer may take one to the real library once the stand-in is gone
        obj.h = None
    del SHAPED[:]


def shaped(cls, **more):
    obj = make(cls, types.SimpleNamespace(h=C.c_void_p(1), _batches=weakref.WeakSet()), C.c_void_p(0x10))
    SHAPED.append(obj)
    for k, v in dict(N=N, K=K, ELL=ELL, LOGB=LOGB, n_lwe=N_LWE, max_keys=2, max_batch=4, **more).items():
        setattr(obj, k, v)
    return obj


def raised(fn):
    with pytest.raises(api.VpbsError) as e:
        fn()
    return str(e.value), getattr(e.value, "status", None)


def test_one_run_body_for_the_bootstrapper_and_the_ring(typed):
    """run, run_from and run_device reach <prefix>_run / _run_from with the table's types -- an empty batch included -- key_of only for the
    ring; a failure names the entry and carries .status where it did before the bodies were shared (not Bootstrapper.run / run_device)"""
    bs, ring = shaped(api.Bootstrapper), shaped(api.KeyRing)
    tv = np.zeros(N, np.uint64)
    for count in (2, 0):
        cts = np.zeros((count, N_LWE + 1), np.uint64)
        for name in ("vpbs_bootstrapper_run", "vpbs_bootstrapper_run_from", "vpbs_keyring_run", "vpbs_keyring_run_from"):
            typed.ret[name] = count
        for obj, ko in ((bs, ()), (ring, ([1] * count,))):
            out_ct, lwe_out = obj.run(cts, *ko, tv)
            assert out_ct.shape == (count, K, N) and lwe_out.shape == (count, N_LWE + 1)
            assert obj.run(cts, *ko, np.zeros((count, N), np.uint64), accumulators=True)[2].shape == (count, N_LWE + 2, K, N)
            assert len(obj.run_from(cts, *ko, [0] * count, None, tv)) == 2
            mine = np.zeros((count, N_LWE + 2, K, N), np.uint64)
            assert obj.run_from(cts, *ko, [1] * count, np.zeros((count, K, N), np.uint64), tv, accumulators=mine)[2] is mine
            assert obj.run_device(4096, count, *ko, 8192, d_lwe_out=12288) is None
    assert typed.calls.count("vpbs_bootstrapper_run") == typed.calls.count("vpbs_keyring_run") == 6
    cts = np.zeros((2, N_LWE + 1), np.uint64)
    typed.ret.update(vpbs_bootstrapper_run=-1, vpbs_bootstrapper_run_from=-1, vpbs_keyring_run=-2, vpbs_keyring_run_from=-2)
    assert raised(lambda: bs.run(cts, tv)) == ("vpbs_bootstrapper_run: status -1: boom", None)
    assert raised(lambda: bs.run_device(1, 2, 3)) == ("vpbs_bootstrapper_run: status -1: boom", None)
    assert raised(lambda: bs.run_from(cts, [0, 0], None, tv)) == ("vpbs_bootstrapper_run_from: status -1: boom", -1)
    assert raised(lambda: ring.run(cts, [0, 1], tv)) == ("vpbs_keyring_run: status -2: boom", -2)
    assert raised(lambda: ring.run_from(cts, [0, 1], [0, 0], None, tv)) == ("vpbs_keyring_run_from: status -2: boom", -2)
    assert raised(lambda: ring.run_device(1, 2, [0, 1], 3)) == ("vpbs_keyring_run: status -2: boom", -2)
    for obj, who, ko in ((bs, "Bootstrapper", ()), (ring, "KeyRing", ([0, 0],))):
        with pytest.raises(ValueError, match=r"%s\.run: expected cts \[count\]\[4\]" % who):
            obj.run(cts[:, :-1], *ko, tv)
        with pytest.raises(ValueError, match=r"%s\.run_from: a row with start > 0 needs acc_in" % who):
            obj.run_from(cts, *ko, [0, 1], None, tv)
    with pytest.raises(ValueError, match="KeyRing: key_of must hold integers"):
        ring.run(cts, None, tv)


def test_one_slot_mixin_for_the_ring_and_the_ring_prover(typed):
    g = K * ELL * K * N
    bsk, ksk = np.zeros((N_LWE, g), np.uint64), np.zeros(g, np.uint64)
    bodies = np.zeros((N_LWE, K * ELL * N), np.uint64), np.zeros(K * ELL * N, np.uint64)
    for obj, name in ((shaped(api.KeyRing), "keyring"), (shaped(api.RingProver), "ring_prover")):
        assert obj.add(bsk, ksk) == 0 and obj.add(4096, 8192, keys_on_device=True) == 0
        assert obj.add_seeded(5, *bodies) == 0 and obj.add_seeded(5, 4096, 8192, bodies_on_device=True) == 0
        assert obj.remove(1) is None
        with pytest.raises(ValueError, match=r"%s\.add: expected bsk \[3\]\[%d\] and ksk \[%d\]" % (type(obj).__name__, g, g)):
            obj.add(bsk[1:], ksk)
        with pytest.raises(ValueError, match="add_seeded: both bsk_bodies and ksk_bodies are needed"):
            obj.add_seeded(5, bodies[0], None)
        text = "boom" if name == "keyring" else ""   # the ring leaves its message with the context, the prover's entries take a buffer
        for entry, call in (("add", lambda: obj.add(bsk, ksk)), ("add_seeded", lambda: obj.add_seeded(5, *bodies)), ("remove", lambda: obj.remove(0))):
            typed.ret["vpbs_%s_%s" % (name, entry)] = -1
            assert raised(call) == ("vpbs_%s_%s: status -1: %s" % (name, entry, text), -1)


def test_one_packing_for_every_verifying_call(typed):
    blobs, tv = [b"ab", b"cde"], np.zeros(N, np.uint64)
    cts, out = np.zeros((2, N_LWE + 1), np.uint64), np.zeros((2, K, N), np.uint64)
    pv, rv, sv = shaped(api.PbsVerifier), shaped(api.RingVerifier), shaped(api.ProofVerifier)
    three = lambda r, shape: len(r) == 3 and all(a.shape == shape and a.dtype == np.uint8 for a in r)
    assert three(pv.verify(blobs, tv, cts, out), (2,)) and three(pv.verify([], tv, cts[:0], out[:0]), (0,))
    assert three(rv.verify(blobs, [0, 1], tv, cts, out), (2,)) and three(rv.verify([], [], tv, cts[:0], out[:0]), (0,))
    assert three(rv.verify(blobs, [0, 1], np.zeros((3, N), np.uint64), cts, out, testv_of=[2, 0]), (2,))
    assert [a.shape for a in sv.verify(blobs)] == [(2,)] * 2 and [a.shape for a in sv.verify([])] == [(0,)] * 2
    with pytest.raises(ValueError, match=r"PbsVerifier\.verify: expected testv \[N\] or \[2\]\[N\], cts \[2\]\[n \+ 1\] and out_cts \[2\]\[K\]\[N\]"):
        pv.verify(blobs, tv, cts[:1], out)
    with pytest.raises(ValueError, match=r"RingVerifier\.verify: 5 proofs exceed max_batch 4"):
        rv.verify([b"x"] * 5, [0] * 5, tv, np.zeros((5, N_LWE + 1), np.uint64), np.zeros((5, K, N), np.uint64))
    typed.ret.update(vpbs_pbs_verifier_run=-1, vpbs_ring_verifier_run=-1, vpbs_proof_verifier_run=-1)
    assert raised(lambda: pv.verify(blobs, tv, cts, out)) == ("vpbs_pbs_verifier_run: status -1", None)
    assert raised(lambda: rv.verify(blobs, [0, 1], tv, cts, out)) == ("vpbs_ring_verifier_run: status -1", -1)
    assert raised(lambda: sv.verify(blobs)) == ("vpbs_proof_verifier_run: status -1", None)
    typed.ret["vpbs_ring_verifier_set_key"] = -1
    assert raised(lambda: rv.set_key(7, np.zeros(4, np.uint64))) == ("vpbs_ring_verifier_set_key: status -1: slot 7 of 2", -1)
    # the aggregates: host statement, device statement, many trees; the aggregator; the program's verifying calls
    shape = types.SimpleNamespace(N=N, K=K, n_lwe=N_LWE, levels=2, c=api.AggregateShapeC())
    av, kh = shaped(api.AggregateVerifier, shape=shape, max_leaves=4, max_aggregates=2), np.zeros((1, 4), np.uint64)
    assert av.root(tv, cts, out, kh, key_of=[0, 0], testv_of=[0, 0]).shape == (4,)
    assert av.root(4096, 8192, 12288, 16384, key_of=[0, 0], on_device=True, count=2, n_testv=1, n_keys=1).shape == (4,)
    assert av.verify(b"xyz", 2, tv, cts, out, kh) == (False, 0) and api.verify_aggregate(shape, b"q", 2, tv, cts, out, kh, key_of=[0, 0]) == (False, 0)
    assert [a.shape for a in av.verify_many([b"x", b"yz"], [1, 1], tv, cts, out, kh)] == [(2,)] * 2
    assert [a.shape for a in av.roots_many([2], tv, cts, out, kh)] == [(1, 4), (1,)]
    assert api.aggregate_root(N, K, N_LWE, np.zeros(68, np.uint64), tv, cts, out, kh).shape == (4,)
    ag = shaped(api.Aggregator, levels=2, max_bytes=64)
    typed.ret["vpbs_aggregator_run"] = 3
    assert ag.aggregate(blobs) == b"\0\0\0" and ag.aggregate_many([blobs, blobs[:1]]) == [None, None]
    typed.ret.update(vpbs_aggregator_run=-4, vpbs_aggregator_run_many=-4)
    assert raised(lambda: ag.aggregate(blobs)) == ("status -4: ", -4) and raised(lambda: ag.aggregate_many([blobs])) == ("status -4: ", -4)
    typed.ret.update(vpbs_pbs_verifier_run=0, vpbs_ring_verifier_run=0)
    prog = shaped(api.Program, n_inputs=1, n_gates=2, n_luts=1, n_wires=3)
    x, tvs = np.zeros((1, N_LWE + 1), np.uint64), np.zeros((1, N), np.uint64)
    assert [a.shape for a in prog.verify(pv, x, tvs, out, blobs)] == [(2,)] * 3
    assert [a.shape for a in prog.verify_batch(rv, x[None], [0], tvs, out[None], [blobs])] == [(1, 2)] * 3
    assert [a.shape for a in prog.verify_aggregate_batch(av, x[None], [0], kh, tvs, out[None], [b"agg"])] == [(1,)] * 2
    typed.ret.update(vpbs_program_verify_batch=-1, vpbs_program_run_batch=-1)
    assert raised(lambda: prog.verify_batch(rv, x[None], [0], tvs, out[None], [blobs])) == ("vpbs_program_verify_batch: status -1: ", -1)
    assert raised(lambda: prog.run_batch(shaped(api.KeyRing), x[None], [0], tvs)) == ("vpbs_program_run_batch: status -1: boom", -1)
    ctx = api.Context.__new__(api.Context)
    ctx.h = C.c_void_p(1)
    assert raised(lambda: ctx._check(-5)) == ("status -5: boom", -5)
    ctx.h = None   # nothing to destroy

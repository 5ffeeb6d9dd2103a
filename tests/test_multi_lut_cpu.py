"""CPU side of multi-output lookup gates (csrc/multi_lut.hip, csrc/program.hip): the host forms (ctx NULL) of the snap, of
sample extraction at a coefficient and of the packed test vector against their restatement in tests/multi_lut_oracle.py, the two mod-switch
properties that make the method work, and the description of a program whose gates have several outputs."""
import ctypes as C

import numpy as np
import pytest

import lwe_client_oracle as LC
import multi_lut_oracle as M
import pbs_batch_oracle as B
import program_oracle as O
from vpbs_amd import api

P = api.P
NAMES = ["vpbs_lwe_snap", "vpbs_lwe_extract_at", "vpbs_lut_testv_multi", "vpbs_program_create_multi", "vpbs_program_wires"]


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for f in (api.lwe_snap, api.lwe_extract_at, api.lut_testv_multi, api.Program.wires, api.Context.lwe_snap, api.Context.lwe_extract_at):
        assert callable(f)


def snap_cases(log_n, theta, rng):
    """0, 1, p - 1, p, 2^64 - 1, 2^63, every block edge (the multiples of 2^t, where r steps, and the half-way points k 2^t + 2^(t - 1),
    where the rounding turns) with its two neighbours, and random words"""
    t = 64 - (log_n + 1) + theta                   # theta = 0: the blocks of the mod switch itself
    words = [0, 1, P - 1, P, (1 << 64) - 1, 1 << 63]
    for k in range(1 << (64 - t)):
        for edge in (k << t, (k << t) + (1 << (t - 1))):
            words += [(edge + d) % (1 << 64) for d in (-1, 0, 1)]
    words += [int(v) for v in rng.integers(0, 1 << 64, size=64, dtype=np.uint64)]
    return words


def test_snap_matches_its_definition_and_keeps_the_mod_switch_aligned():
    """for log_N 1 .. 11 and every theta < L = log_N + 1: the definition; mod_switch(snap(w)) = r 2^theta mod 2N and
    mod_switch(-snap(w)) = -r 2^theta mod 2N (the body's path through step 0); snap(w) at most 2^(t - 1) away from w mod 2^64"""
    rng = np.random.default_rng(64)
    cases = 0
    for log_n in range(1, 12):
        two_n = 2 << log_n
        for theta in range(0, log_n + 1):
            words = snap_cases(log_n, theta, rng)
            got = api.lwe_snap(1 << log_n, theta, np.array(words, np.uint64))
            cases += len(words)
            for w, g in zip(words, got.tolist()):
                assert g == M.snap(w, log_n, theta), (log_n, theta, hex(w), hex(g))
                assert g < P
                if theta == 0:
                    assert g == w % P if w >= P else g == w           # only reduces
                    continue
                r, t = M.snap_r(w, log_n, theta)
                assert g == (r << t) % (1 << 64) and (g == 0) == (r in (0, 1 << (log_n + 1 - theta)))
                assert M.mod_switch(g, log_n) % two_n == (r << theta) % two_n
                assert M.mod_switch((P - g) % P, log_n) % two_n == -(r << theta) % two_n
                d = (g - w % P) % (1 << 64)
                assert min(d, (1 << 64) - d) <= 1 << (t - 1)
    assert cases > 100000


def test_snap_refusals_and_shapes():
    w = np.arange(12, dtype=np.uint64).reshape(3, 4)
    assert api.lwe_snap(8, 2, w).shape == (3, 4)
    assert api.lwe_snap(8, 0, np.zeros(0, np.uint64)).size == 0
    for N, theta in ((8, 4), (2, 2), (4096, 1), (1, 0)):
        with pytest.raises(api.VpbsError, match="status -1"):
            api.lwe_snap(N, theta, w)
    L = api.lib()
    assert L.vpbs_lwe_snap(None, 3, 1, None, 4, w.ctypes.data, 0) == -1
    assert L.vpbs_lwe_snap(None, 3, 1, w.ctypes.data, 4, w.ctypes.data, 1) == -1     # device pointers need a context


def test_the_packed_test_vector():
    rng = np.random.default_rng(5)
    for N, p, s in ((8, 2, 2), (64, 2, 4), (64, 4, 8), (128, 2, 32), (16, 1, 8), (1024, 2, 8)):
        tables = rng.integers(0, 2 * p, size=(s, p), dtype=np.uint64)
        delta = int(rng.integers(1, P, dtype=np.uint64))
        got, d = api.lut_testv_multi(N, p, tables, delta)
        assert d == delta and got.tolist() == M.lut_testv_multi(N, p, tables.tolist(), delta)
        Ts = [api.lut_testv(N, p, t, delta)[0] for t in tables]
        for j in range(s):                                         # slot j of every group holds table j's entry of that group
            assert (got[j::s] == Ts[j][0::s]).all() and all((Ts[j][q::s] == Ts[j][0::s]).all() for q in range(s))
    # one table is vpbs_lut_testv, default delta included, and then p may go up to N
    table = np.array([1, 3, 0, 2], np.uint64)
    assert api.lut_testv_multi(64, 4, table.reshape(1, 4))[0].tolist() == api.lut_testv(64, 4, table)[0].tolist()
    assert api.lut_testv_multi(64, 4, table.reshape(1, 4))[1] == api.lut_testv(64, 4, table)[1]
    ident = np.arange(8, dtype=np.uint64).reshape(1, 8)
    assert api.lut_testv_multi(8, 8, ident, 3)[0].tolist() == api.lut_testv(8, 8, ident[0], 3)[0].tolist() == LC.lut_testv(8, 8, ident[0], 3)


def test_the_packed_test_vector_refusals():
    ok = np.zeros((2, 2), np.uint64)
    api.lut_testv_multi(8, 2, ok, 1)                               # s 2 p = 8 = N: the last shape that fits
    with pytest.raises(api.VpbsError):
        api.lut_testv_multi(8, 2, np.zeros((4, 2), np.uint64), 1)  # s 2 p = 16 > N: the half-block shift would leave the groups
    with pytest.raises(api.VpbsError):
        api.lut_testv_multi(8, 4, np.zeros((2, 4), np.uint64), 1)
    bad = ok.copy()
    bad[1, 1] = 4                                                  # an entry of the second table at 2 p
    out = np.full(8, 7, np.uint64)
    assert api.lib().vpbs_lut_testv_multi(3, 2, 1, api._ptr(bad.reshape(-1)), 1, api._ptr(out)) == -1 and (out == 7).all()
    with pytest.raises(api.VpbsError):
        api.lut_testv_multi(16, 3, np.zeros((2, 3), np.uint64), 1)  # p not a power of two
    with pytest.raises(ValueError):
        api.lut_testv_multi(16, 2, np.zeros((3, 2), np.uint64), 1)  # three tables
    assert api.lib().vpbs_lut_testv_multi(3, 2, 4, api._ptr(ok.reshape(-1)), 1, api._ptr(out)) == -1      # log_slots > log_N


@pytest.mark.parametrize("log_n,K,n_lwe", [(3, 2, 6), (3, 2, 8), (3, 3, 12), (3, 3, 16), (2, 3, 5), (1, 2, 2)])
def test_extraction_at_a_coefficient(log_n, K, n_lwe):
    """j = 0, 1, N - 1 (and all between); K = 3 with n_lwe > N crosses a polynomial; zeros stay zeros; j = 0 is partial_sample_extract"""
    N = 1 << log_n
    rng = np.random.default_rng(log_n * 10 + K)
    glwe = rng.integers(0, P, size=(3, K, N), dtype=np.uint64)
    glwe[1, 0, ::2] = 0
    index = np.array([j for _ in range(3) for j in range(N)], np.uint32)
    src = np.array([c for c in range(3) for _ in range(N)], np.uint32)
    got = api.lwe_extract_at(glwe, n_lwe, index, src)
    assert got.shape == (3 * N, n_lwe + 1)
    for row, j, c in zip(got.tolist(), index.tolist(), src.tolist()):
        assert row == M.extract_at(B.glwe_list(glwe[c]), n_lwe, j), (j, c)
        if j == 0:
            assert row == B.extract(B.glwe_list(glwe[c]), n_lwe)
    # the rows may name the GLWEs in any order and more than once; one [K][N] array is one GLWE
    assert api.lwe_extract_at(glwe, n_lwe, [N - 1, 1, N - 1], [2, 0, 2]).tolist() == [got[2 * N + N - 1].tolist(), got[1].tolist(), got[3 * N - 1].tolist()]
    assert api.lwe_extract_at(glwe[1], n_lwe, [1], [0]).tolist() == [got[N + 1].tolist()]
    assert api.lwe_extract_at(glwe, n_lwe, [], []).shape == (0, n_lwe + 1)


def test_extraction_refusals():
    glwe = np.zeros((2, 2, 8), np.uint64)
    for index, src in (([8], [0]), ([0, 7, 9], [0, 1, 1]), ([0], [2])):
        with pytest.raises(api.VpbsError, match="status -1"):
            api.lwe_extract_at(glwe, 6, index, src)
    with pytest.raises(api.VpbsError):
        api.lwe_extract_at(glwe, 9, [0], [0])                      # n_lwe above (K - 1) N
    with pytest.raises(ValueError):
        api.lwe_extract_at(glwe, 6, [0, 1], [0])


# 2 inputs (wires 0 1); gate 0 (1 slot, wires 2), gate 1 (2 slots, wires 3 4), gate 2 (4 slots, 3 outputs, wires 5 6 7), gate 3 reads wire 4
# (output 1 of gate 1) and wire 7 (output 2 of gate 2): level 2; gate 4 (snapped, one output, wire 9) reads wire 8: level 3
MIXED = [([(0, 1)], 0, 0),
         ([(1, 1)], 0, 1, 1, 2),
         ([(0, 1), (1, 1)], 3, 2, 2, 3),
         ([(4, 1), (7, P - 1)], 0, 0, 0, 1),
         ([(8, 2)], 0, 1, 1, 1)]


def test_wire_numbering_and_levels_of_a_host_only_program():
    assert M.out_first(MIXED) == [0, 1, 3, 6, 7, 8] and M.levels(2, MIXED) == ([1, 1, 1, 2, 3], 3)
    for form in (MIXED, M.csr(MIXED)):
        prog = api.Program(None, 2, form, 3)
        first, n_wires = prog.wires()
        assert first.tolist() == [0, 1, 3, 6, 7, 8] and n_wires == 10 == prog.n_wires
        lv, n = prog.levels()
        assert lv.tolist() == [1, 1, 1, 2, 3] and n == 3
        prog.close()
    # a seeded DAG whose gates get 1 .. 4 outputs: the levels follow the wires' owners
    rng = np.random.default_rng(11)
    gates, n_wires = [], 3
    for g in range(60):
        theta = int(rng.integers(0, 3))
        m = int(rng.integers(1, (1 << theta) + 1))
        terms = [(int(rng.integers(0, n_wires)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(int(rng.integers(0, 4)))]
        gates.append((terms, int(rng.integers(0, P, dtype=np.uint64)), 0, theta, m))
        n_wires += m
    prog = api.Program(None, 3, gates, 1)
    assert prog.wires()[0].tolist() == M.out_first(gates) and prog.wires()[1] == n_wires
    want, n_levels = M.levels(3, gates)
    assert prog.levels()[0].tolist() == want and prog.levels()[1] == n_levels and n_levels > 3
    prog.close()


def test_a_plain_program_and_its_0_1_form_are_the_same_description():
    plain = O.random_dag(np.random.default_rng(200), 5, 80, 3)
    a, b = api.Program(None, 5, plain, 3), api.Program(None, 5, [g + (0, 1) for g in plain], 3)
    assert a.levels()[0].tolist() == b.levels()[0].tolist() and a.levels()[1] == b.levels()[1]
    assert a.wires()[0].tolist() == b.wires()[0].tolist() == list(range(81)) and a.wires()[1] == b.wires()[1] == 85
    a.close()
    b.close()


def refused(gates, gate, word, n_luts=3):
    with pytest.raises(api.VpbsError) as e:
        api.Program(None, 2, gates, n_luts)
    text = str(e.value)
    assert "status -1" in text and ("gate %d" % gate) in text and word in text, text


def test_every_refusal_names_its_gate():
    g = [list(x) for x in MIXED]
    g[2][4] = 0
    refused(g, 2, "gate_outputs")
    g = [list(x) for x in MIXED]
    g[2][4] = 5                                                    # 5 outputs, 4 slots
    refused(g, 2, "gate_outputs")
    g = [list(x) for x in MIXED]
    g[1][3], g[1][4] = 0, 2                                        # two outputs without a snap
    refused(g, 1, "gate_outputs")
    g = [list(x) for x in MIXED]
    g[3][0] = [(8, 1)]                                             # gate 3 reads its own output: wires below 2 + out_first[3] = 8 only
    refused(g, 3, "topological")
    g = [list(x) for x in MIXED]
    g[1][0] = [(3, 1)]                                             # gate 1 reads its own first output
    refused(g, 1, "topological")
    g = [list(x) for x in MIXED]
    g[4][2] = 3
    refused(g, 4, "gate_lut")
    g = [list(x) for x in MIXED]
    g[0] = g[0] + [40, 1]
    refused(g, 0, "gate_log_slots")
    # wire 7 exists only because gate 2 has three outputs: with two it is gate 3's own output
    g = [list(x) for x in MIXED]
    g[2][4] = 2
    refused(g, 3, "topological")
    # the arrays of the new call may not be missing
    d = api.ProgramDescC(1, 1, 1, 0, api._ptr(np.zeros(2, np.uint64)), None, None, api._ptr(np.zeros(1, np.uint64)),
                         np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)))
    out, err = C.c_void_p(), C.create_string_buffer(256)
    assert api.lib().vpbs_program_create_multi(None, C.byref(d), None, None, C.byref(out), err, 256) == -1 and not out.value
    assert api.lib().vpbs_program_wires(None, None) == -1


def test_program_batch_args_learns_the_row_count():
    x, tv = np.zeros((3, 2, 7), np.uint64), np.zeros((3, 8), np.uint64)
    assert len(api.program_batch_args(2, 6, 8, 3, 4, x, [0, 1, 0], tv)) == 3
    assert api.program_batch_args(2, 6, 8, 3, 4, x, [0, 1, 0], tv, gate_outputs=[g[4] for g in M.norm(MIXED)])[3] == (3, 10, 7)
    with pytest.raises(ValueError, match="gate 1"):
        api.program_batch_args(2, 6, 8, 3, 4, x, [0, 1, 0], tv, gate_outputs=[1, 0, 2])

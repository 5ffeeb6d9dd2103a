"""verifier timing on a full-size (2^15) step proof produced on the GPU: vpbs_verify_step on the host (default), or with
--device --batch B the device batch verifier (vpbs_proof_verifier_run, wall clock including the upload, plus device events) against the
host verifier on 16 threads over the same B serialised proofs, five alternating repetitions each: the 2^15 synthetic proof (fri_only:
its wires satisfy no gate), or with --paper proofs of the exported step circuit at N = 1024 under the full check"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, vpbs_amd
from vpbs_amd import api, synth
import bench
args = sys.argv[1:]
device_mode = "--device" in args
batch = int(args[args.index("--batch") + 1]) if "--batch" in args else 1
log_n = 15
ctx = vpbs_amd.Context(0, log_n_max=16)
gates = api.GateSet(bench.GATES)
inputs = synth.step_inputs(log_n, cols=bench.COLS)
cs = ctx.commit_values(inputs["constants_sigmas"])
pis = synth.field_elements(0xABCD, 77)
sig = np.ascontiguousarray(inputs["constants_sigmas"][bench.N_CONSTANTS:])
digest = np.array([11, 22, 33, 44], np.uint64)
si = ctx.make_step_inputs(log_n, inputs["wires"], None, None, cs, digest, pis, sigmas=sig, n_routed=80, n_constants=bench.N_CONSTANTS, gates=gates)
proof = ctx.prove_step(si)
cap = cs.cap()
ncols = [bench.COLS["constants_sigmas"], 135, 20, 16]
for check in (False, True):
    t = time.perf_counter()
    for _ in range(5):
        ok = api.verify_step(proof, cap, ncols, digest, pis, log_n, check_permutation=check, n_constants=bench.N_CONSTANTS, n_routed=80,
                             gates=gates if check else None)
    dt = (time.perf_counter() - t) / 5
    print("verify_step (FRI%s): %.2f ms, accepted=%s" % (" + vanishing identity with gates" if check else " only", dt * 1e3, ok))



def device_against_host(what, blobs, pv, host_one):
    """five alternating runs: the device batch (wall clock of vpbs_proof_verifier_run, upload included) and the host verifier on 16
    threads over the same blobs; then one device run with event timing around every kernel -> one JSON line"""
    import json
    from concurrent.futures import ThreadPoolExecutor
    buf, offs = api.pack_proofs(blobs)
    pv.verify_packed(buf, offs)   # warm-up: first launches, pinned staging
    dev_ms, host_ms = [], []
    with ThreadPoolExecutor(max_workers=16) as pool:
        for _ in range(5):
            t = time.perf_counter()
            v, _ = pv.verify_packed(buf, offs)
            dev_ms.append((time.perf_counter() - t) * 1e3)
            assert v.all()
            t = time.perf_counter()
            ok = list(pool.map(host_one, blobs))
            host_ms.append((time.perf_counter() - t) * 1e3)
            assert all(ok)
    ctx.timing_enable(1)
    pv.verify_packed(buf, offs)
    kernels = ctx.timing_report()
    ctx.timing_enable(0)
    med = lambda x: sorted(x)[len(x) // 2]
    print(json.dumps({"what": what, "batch": len(blobs), "bytes_per_proof": len(blobs[0]), "device_ms_per_run_wall": med(dev_ms),
                      "host_16_threads_ms": med(host_ms), "speedup": med(host_ms) / med(dev_ms), "device_runs_ms": dev_ms,
                      "host_runs_ms": host_ms, "device_kernels": kernels}))


if device_mode and "--paper" not in args:
    nconst = bench.N_CONSTANTS
    blob = ctx.step_proof_to_bytes(si, nconst, proof)
    # the synthetic wires satisfy no gate, so both sides run transcript + PoW + FRI + Merkle paths (fri_only): the work that accepts them
    pv = api.ProofVerifier(ctx, cap, ncols, digest, log_n, check_permutation=False, max_batch=batch, max_public_inputs=len(pis))

    def host_one(b):
        p, pi = api.step_proof_from_bytes(b, ncols, log_n, nconst, max_public_inputs=len(pis))
        return api.verify_step_fri_only(p, cap, ncols, digest, pi, log_n)
    device_against_host("fri_only: synthetic 2^%d step proofs" % log_n, [blob] * batch, pv, host_one)
    pv.close()

if device_mode and "--paper" in args:
    # --paper: the exported step circuit at N = 1024 (the paper's parameters), 8 distinct proofs of satisfied witnesses, FULL check (gate
    # constraints and permutation argument at zeta included) on both sides
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_circuits
    from vpbs_amd import circuit_file
    d = circuit_file.load(export_circuits.ensure_step_circuit(1024, 2, 4, 5, 728))
    plan = d.circuit.witness_plan(d.preset_pos)
    sigma = d.circuit.sigma_values()
    pcs = ctx.commit_values(np.concatenate([d.constants, sigma]))
    pcap, pncols = pcs.cap(), [d.n_constants + 80, 135, 20, 16]
    distinct = []
    for seed in range(8):
        v = np.random.default_rng(seed).integers(0, api.P, size=len(d.preset_pos), dtype=np.uint64)
        v[len(d.preset_pos) - 10] = 1 + seed
        w = plan.run(v)
        ppis = np.array([w[c][r] for c, r in d.pi_pos], np.uint64)
        psi = ctx.make_step_inputs(d.log_n, w, None, None, pcs, digest, ppis, sigmas=sigma, n_routed=80, n_constants=d.n_constants,
                                   gates=d.gates)
        distinct.append(ctx.step_proof_to_bytes(psi, d.n_constants, ctx.prove_step(psi)))
    plan.free()
    n_pi = len(d.pi_pos)
    pv = api.ProofVerifier(ctx, pcap, pncols, digest, d.log_n, n_constants=d.n_constants, n_routed=80, gates=d.gates, max_batch=batch,
                           max_public_inputs=n_pi)

    def host_one(b):
        p, pi = api.step_proof_from_bytes(b, pncols, d.log_n, d.n_constants, max_public_inputs=n_pi)
        return api.verify_step(p, pcap, pncols, digest, pi, d.log_n, n_constants=d.n_constants, n_routed=80, gates=d.gates)
    device_against_host("full check: step circuit at N = 1024 (2^%d rows), 8 distinct proofs" % d.log_n,
                        [distinct[k % 8] for k in range(batch)], pv, host_one)
    pv.close()

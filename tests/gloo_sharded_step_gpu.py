"""Run by test_gpu_parity.py::test_sharded_step_proof_multi_rank, every rank on the one GPU of the test box: a step proof with every
commitment coset-sharded over the ranks is bit-identical, on every rank, to the single-GPU step proof, and verifies under the oracle's
verifier.

Two ways to run the ranks, the same checks and the same sharded prover (vpbs_prove_step_sharded through host-callback collectives):
  * under torch.distributed.run: one process per rank, the collectives over gloo (sharding.make_comm / sharding.sharded_commit);
  * `gloo_sharded_step_gpu.py --threads WORLD`: WORLD ranks as threads of ONE process, each with its own context, the collectives
    exchanged in memory (ThreadRanks) with the semantics of the gloo callbacks -- for worlds whose processes a shared card could not
    hold (at most six processes may have it open)."""
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "circuitgen")]
import step_oracle  # noqa: E402
import vpbs_amd  # noqa: E402
from vpbs_amd import api, sharding, synth  # noqa: E402


class GlooRank:
    """this process is one rank of the torch.distributed (gloo) group"""

    def __init__(self):
        import torch.distributed as dist
        self.dist = dist
        dist.init_process_group("gloo")
        self.rank, self.world = dist.get_rank(), dist.get_world_size()

    def sharded_commit(self, ctx, d_values_ptr, ncols, log_n):
        return sharding.sharded_commit(ctx, d_values_ptr, ncols, log_n)

    def make_comm(self, stage_words):
        return sharding.make_comm(stage_words=stage_words)

    def barrier(self):
        self.dist.barrier()

    def close(self):
        self.dist.destroy_process_group()


class ThreadRanks:
    """`world` ranks as threads of one process: what gloo's all_gather / all_reduce do between processes, done in memory.  Every collective
    is an exchange: each rank posts its part, all meet, each reads every part, all meet again before a slot can be reused."""

    def __init__(self, world):
        self.world = world
        self.meet = threading.Barrier(world, timeout=600)
        self.slots = [None] * world
        self.stage = [None] * world

    def exchange(self, rank, part):
        self.slots[rank] = part
        self.meet.wait()
        parts = list(self.slots)
        self.meet.wait()
        return parts

    def rank_view(self, rank):
        return ThreadRank(self, rank)


class ThreadRank:
    def __init__(self, group, rank):
        self.group, self.rank, self.world = group, rank, group.world

    def sharded_commit(self, ctx, d_values_ptr, ncols, log_n):
        """sharding.sharded_commit without torch.distributed: this rank's cosets, then the cap entries of all ranks in rank order"""
        batch, local_cap = ctx.commit_sharded_dev(d_values_ptr, ncols, log_n, self.rank, self.world)
        return batch, np.concatenate(self.group.exchange(self.rank, np.ascontiguousarray(local_cap)), axis=0)

    def make_comm(self, stage_words):
        """sharding.make_comm's callbacks (all-gather, wrapping u64 sum, device all-gather through the staging buffers) between threads"""
        g, rank, world = self.group, self.rank, self.world

        def _allgather(user, local, local_words, full):
            try:
                src = np.ctypeslib.as_array(local, shape=(local_words,)).copy()
                dst = np.ctypeslib.as_array(full, shape=(world * local_words,))
                dst[:] = np.concatenate(g.exchange(rank, src))
                return 0
            except Exception:  # must not unwind through the C frame
                import traceback
                traceback.print_exc()
                g.meet.abort()
                return -1

        def _allreduce(user, inout, words):
            try:
                buf = np.ctypeslib.as_array(inout, shape=(words,))
                total = np.zeros(words, np.uint64)
                for part in g.exchange(rank, buf.copy()):
                    total += part                     # wrapping u64 sum, as the int64 sum of gloo
                buf[:] = total
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                g.meet.abort()
                return -1

        local_t = torch.zeros(stage_words, dtype=torch.int64, device="cuda")
        full_t = torch.zeros(stage_words * world, dtype=torch.int64, device="cuda")
        g.stage[rank] = local_t

        def _allgather_dev(user, local_words):
            try:
                torch.cuda.synchronize()              # the library has synchronised its stream; the staging buffers are final
                g.meet.wait()
                for r in range(world):
                    full_t[r * local_words:(r + 1) * local_words].copy_(g.stage[r][:local_words])
                torch.cuda.synchronize()
                g.meet.wait()                         # nobody writes its staging buffer again before every rank has read it
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                g.meet.abort()
                return -1

        comm = api.CommC()
        comm.rank, comm.world = rank, world
        comm.allgather = api.ALLGATHER_FN(_allgather)
        comm.allreduce_sum = api.ALLREDUCE_FN(_allreduce)
        comm.user = None
        comm.allgather_dev = api.ALLGATHER_DEV_FN(_allgather_dev)
        comm.d_stage_local = local_t.data_ptr()
        comm.d_stage_full = full_t.data_ptr()
        comm.stage_capacity_words = stage_words
        comm._keep = (_allgather, _allreduce, _allgather_dev, comm.allgather, comm.allreduce_sum, comm.allgather_dev, local_t, full_t)
        return comm

    def barrier(self):
        self.group.meet.wait()

    def close(self):
        pass


def prove_and_check(ranks, log_n):
    rank, world = ranks.rank, ranks.world
    torch.cuda.set_device(0)
    ctx = vpbs_amd.Context(0, log_n_max=16)
    inputs = synth.step_inputs(log_n)
    digest = np.array([5, 6, 7, 8], np.uint64)
    pis = synth.field_elements(4242, 33)
    n_constants, n_routed = 5, 80
    sig = np.ascontiguousarray(inputs["constants_sigmas"][n_constants:n_constants + n_routed])
    # reference: the unsharded proof on this rank
    cs_full = ctx.commit_values(inputs["constants_sigmas"])
    si_full = ctx.make_step_inputs(log_n, inputs["wires"], None, inputs["quotient"], cs_full, digest, pis, sigmas=sig, n_routed=n_routed)
    want = ctx.prove_step(si_full)
    # sharded: constants_sigmas committed per rank, then the sharded step
    dev_cs = torch.from_numpy(inputs["constants_sigmas"].view(np.int64)).cuda()
    torch.cuda.synchronize()
    cs_shard, cs_cap = ranks.sharded_commit(ctx, dev_cs.data_ptr(), 85, log_n)
    assert (cs_cap == cs_full.cap()).all()
    comm = ranks.make_comm((2 << (log_n + 3)) // world)
    si = ctx.make_step_inputs(log_n, inputs["wires"], None, inputs["quotient"], cs_shard, digest, pis, sigmas=sig, n_routed=n_routed)
    got = ctx.prove_step(si, comm)
    for key in ("caps", "challenges", "openings", "fri"):
        assert (got[key] == want[key]).all(), (rank, key)
    assert got["challenger"].state_words() == want["challenger"].state_words()
    assert step_oracle.verify_step(got, cs_cap, [85, 135, 20, 16], digest, pis, log_n)
    # a replicated (unsharded) constants_sigmas batch is accepted too: rank 0 answers its queries
    si2 = ctx.make_step_inputs(log_n, inputs["wires"], None, inputs["quotient"], cs_full, digest, pis, sigmas=sig, n_routed=n_routed)
    got2 = ctx.prove_step(si2, comm)
    assert (got2["fri"] == want["fri"]).all()
    # quotient evaluated on the device: sharded (values all-gathered between the ranks) == single GPU
    si3 = ctx.make_step_inputs(log_n, inputs["wires"], None, None, cs_full, digest, pis, sigmas=sig, n_routed=n_routed, n_constants=n_constants)
    want3 = ctx.prove_step(si3)
    si4 = ctx.make_step_inputs(log_n, inputs["wires"], None, None, cs_shard, digest, pis, sigmas=sig, n_routed=n_routed, n_constants=n_constants)
    got4 = ctx.prove_step(si4, comm)
    for key in ("caps", "openings", "fri"):
        assert (got4[key] == want3[key]).all(), (rank, "device quotient", key)
    # ... and with the gate constraints of all 14 gate types in the quotient (each rank evaluates them on its own cosets)
    gates = vpbs_amd.api.GateSet(["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon", "poseidon_mds", "arithmetic_ext",
                                  "mul_ext", "reducing", "reducing_ext", ("random_access", 4), "exponentiation", "coset_interpolation"])
    assert gates.num_selectors + gates.num_constants <= n_constants + 1
    nc6 = gates.num_selectors + gates.num_constants
    cs6_vals = np.ascontiguousarray(synth.trace(0xBEEF, nc6 + n_routed, log_n))
    sig6 = np.ascontiguousarray(cs6_vals[nc6:])
    cs6_full = ctx.commit_values(cs6_vals)
    dev_cs6 = torch.from_numpy(cs6_vals.view(np.int64)).cuda()
    torch.cuda.synchronize()
    cs6_shard, cs6_cap = ranks.sharded_commit(ctx, dev_cs6.data_ptr(), nc6 + n_routed, log_n)
    si5 = ctx.make_step_inputs(log_n, inputs["wires"], None, None, cs6_full, digest, pis, sigmas=sig6, n_routed=n_routed, n_constants=nc6, gates=gates)
    want5 = ctx.prove_step(si5)
    si6 = ctx.make_step_inputs(log_n, inputs["wires"], None, None, cs6_shard, digest, pis, sigmas=sig6, n_routed=n_routed, n_constants=nc6, gates=gates)
    got6 = ctx.prove_step(si6, comm)
    for key in ("caps", "openings", "fri"):
        assert (got6[key] == want5[key]).all(), (rank, "device quotient with gates", key)
    assert not (want5["caps"][2] == want3["caps"][2]).all()   # the gate terms really are in the quotient
    ranks.barrier()
    ctx.close()


def main():
    log_n = int(os.environ.get("VPBS_TEST_LOG_N", "10"))
    if len(sys.argv) == 3 and sys.argv[1] == "--threads":
        group = ThreadRanks(int(sys.argv[2]))
        errs = []

        def run(r):
            try:
                prove_and_check(group.rank_view(r), log_n)
            except BaseException as e:   # noqa: BLE001  (the other ranks must not wait for this one)
                errs.append((r, e))
                group.meet.abort()
        threads = [threading.Thread(target=run, args=(r,)) for r in range(group.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errs:
            errs.sort(key=lambda x: isinstance(x[1], threading.BrokenBarrierError))   # the first real failure, not its echoes
            raise errs[0][1]
        world = group.world
    else:
        ranks = GlooRank()
        prove_and_check(ranks, log_n)
        world = ranks.world
        ranks.close()
        if ranks.rank != 0:
            return
    print("SHARDED_STEP_OK world=%d log_n=%d" % (world, log_n))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Which hardware queue did each host thread's kernels run on?  Reads the kernel-trace CSV of

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 20 --warmup 4

(no counters in that run) and prints, and with --out writes as JSON, per queue id:
  * the host threads whose leaf_hash_kernel dispatches ran there, with their dispatch counts -- a thread that launches leaf_hash_kernel proves
    (three launches per step proof); threads below --min-dispatches launches in all are listed under "setup_threads" and not counted (the
    main thread commits every chain's circuit constants on that chain's stream before the chain threads start);
  * the sync_word_kernel dispatches of threads that launched no leaf_hash_kernel at all: the upload threads (vpbs_device_upload_bg waits
    through a marker on the upload stream).
Plain CSV arithmetic: nothing but Queue_Id, Thread_Id and Kernel_Name of each row is looked at.

usage: queue_map.py TRACE.csv | DIR  [--min-dispatches N] [--out FILE.json]
A directory stands for the newest *kernel_trace.csv below it.
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys


def find_trace(path):
    if os.path.isfile(path):
        return path
    found = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        raise SystemExit("queue_map.py: no *kernel_trace.csv below %s" % path)
    return max(found, key=os.path.getmtime)


def short(kernel_name):
    """vpbs::(anonymous namespace)::leaf_hash_kernel<8u>(unsigned long*) [clone .kd] -> leaf_hash_kernel"""
    head = kernel_name.replace("(anonymous namespace)", "").split("<")[0].split("(")[0].split("[")[0]
    words = head.split("::")[-1].split()
    return words[-1].replace(".kd", "") if words else kernel_name


def queue_map(rows, min_dispatches=1):
    """rows: dicts with Queue_Id, Thread_Id, Kernel_Name.  Returns the table described in the module's docstring."""
    leaf = collections.defaultdict(collections.Counter)     # thread -> queue -> leaf_hash_kernel dispatches
    marks = collections.defaultdict(collections.Counter)    # thread -> queue -> sync_word_kernel dispatches
    for r in rows:
        k = short(r["Kernel_Name"])
        if k == "leaf_hash_kernel":
            leaf[r["Thread_Id"]][r["Queue_Id"]] += 1
        elif k == "sync_word_kernel":
            marks[r["Thread_Id"]][r["Queue_Id"]] += 1
    provers = {t: q for t, q in leaf.items() if sum(q.values()) >= min_dispatches}
    setup = {t: dict(q) for t, q in leaf.items() if t not in provers}
    queues = collections.defaultdict(lambda: {"prover_threads": 0, "leaf_hash_dispatches": {}, "upload_threads": 0, "upload_markers": {}})
    for t, q in provers.items():
        for qid, n in q.items():
            queues[qid]["leaf_hash_dispatches"][t] = n
            queues[qid]["prover_threads"] += 1
    uploaders = {t: q for t, q in marks.items() if t not in leaf}
    for t, q in uploaders.items():
        for qid, n in q.items():
            queues[qid]["upload_markers"][t] = n
            queues[qid]["upload_threads"] += 1
    prover_queues = sorted(q for q, v in queues.items() if v["prover_threads"])
    upload_queues = sorted(q for q, v in queues.items() if v["upload_threads"])
    return {
        "queues": {q: queues[q] for q in sorted(queues)},
        "prover_threads": len(provers),
        "prover_queue_ids": prover_queues,
        "most_provers_on_one_queue": max([queues[q]["prover_threads"] for q in prover_queues], default=0),
        "prover_threads_on_more_than_one_queue": sorted(t for t, q in provers.items() if len(q) > 1),
        "upload_threads": len(uploaders),
        "upload_marker_queue_ids": upload_queues,
        "upload_markers_on_a_prover_queue": sorted(set(prover_queues) & set(upload_queues)),
        "setup_threads": setup,
        "min_dispatches": min_dispatches,
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="kernel-trace CSV of rocprofv3, or a directory that holds one")
    ap.add_argument("--min-dispatches", type=int, default=1, help="leaf_hash_kernel launches a thread needs to count as a proving thread")
    ap.add_argument("--out", default=None, help="write the table to this file as JSON as well")
    args = ap.parse_args(argv)
    path = find_trace(args.trace)
    with open(path, newline="") as f:
        table = queue_map(csv.DictReader(f), args.min_dispatches)
    table["trace"] = os.path.basename(path)
    text = json.dumps(table, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""tools/queue_map.py on made-up kernel-trace rows: which thread's leaf_hash_kernel dispatches ran on which queue, and where the markers of
the threads that only upload went."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import queue_map  # noqa: E402

LEAF = "void vpbs::(anonymous namespace)::leaf_hash_kernel<8u>(unsigned long const*, unsigned long*) [clone .kd]"
MARK = "vpbs::sync_word_kernel(unsigned long volatile*, unsigned long)"
OTHER = "vpbs::(anonymous namespace)::ntt_radix16_kernel(unsigned long*)"


def rows(spec):
    return [{"Queue_Id": str(q), "Thread_Id": str(t), "Kernel_Name": k} for q, t, k, n in spec for _ in range(n)]


def test_short_names():
    assert queue_map.short(LEAF) == "leaf_hash_kernel"
    assert queue_map.short(MARK) == "sync_word_kernel"
    assert queue_map.short("leaf_hash_kernel.kd") == "leaf_hash_kernel"
    assert queue_map.short(OTHER) == "ntt_radix16_kernel"


def test_provers_uploaders_and_the_setup_thread():
    # threads 11-14 prove (two per queue on queues 1 and 3, their own markers beside them), 21 and 22 only upload (queue 2; 22 once on queue 1
    # as well), thread 1 committed something on every prover queue before the chains started
    spec = [(1, 11, LEAF, 60), (1, 11, MARK, 200), (1, 12, LEAF, 60), (3, 13, LEAF, 60), (3, 14, LEAF, 57), (3, 14, OTHER, 500),
            (2, 21, MARK, 20), (2, 22, MARK, 19), (1, 22, MARK, 1), (1, 1, LEAF, 2), (3, 1, LEAF, 2), (0, 1, OTHER, 9)]
    m = queue_map.queue_map(rows(spec), min_dispatches=40)
    assert m["prover_threads"] == 4 and m["prover_queue_ids"] == ["1", "3"] and m["most_provers_on_one_queue"] == 2
    assert m["prover_threads_on_more_than_one_queue"] == []
    assert m["queues"]["1"]["leaf_hash_dispatches"] == {"11": 60, "12": 60} and m["queues"]["3"]["leaf_hash_dispatches"] == {"13": 60, "14": 57}
    assert m["upload_threads"] == 2 and m["upload_marker_queue_ids"] == ["1", "2"] and m["upload_markers_on_a_prover_queue"] == ["1"]
    assert m["queues"]["2"]["upload_markers"] == {"21": 20, "22": 19} and m["queues"]["1"]["upload_markers"] == {"22": 1}
    assert m["setup_threads"] == {"1": {"1": 2, "3": 2}}
    assert "0" not in m["queues"]                      # a queue with neither is not listed
    # without the threshold the setup thread counts as a prover that moved between queues
    m1 = queue_map.queue_map(rows(spec))
    assert m1["prover_threads"] == 5 and m1["prover_threads_on_more_than_one_queue"] == ["1"]


def test_command_line_reads_the_newest_trace_of_a_directory(tmp_path, capsys):
    d = tmp_path / "out" / "host" / "123"
    d.mkdir(parents=True)
    with open(d / "123_kernel_trace.csv", "w", newline="") as f:
        w = csv.DictWriter(f, ["Kind", "Queue_Id", "Thread_Id", "Kernel_Name"])
        w.writeheader()
        for r in rows([(4, 7, LEAF, 3), (5, 8, MARK, 2)]):
            w.writerow(dict(r, Kind="KERNEL_DISPATCH"))
    out = tmp_path / "map.json"
    assert queue_map.main([str(tmp_path / "out"), "--out", str(out)]) == 0
    printed = json.loads(capsys.readouterr().out)
    assert printed == json.load(open(out)) and printed["trace"] == "123_kernel_trace.csv"
    assert printed["prover_queue_ids"] == ["4"] and printed["upload_marker_queue_ids"] == ["5"]

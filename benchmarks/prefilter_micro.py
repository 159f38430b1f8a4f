"""In-process cost per event of the benchmark's filter shape: the critical
filter plus a namespace filter over half of the corpus's namespaces, a native
notifier core and ``validate: payload`` — the shape in which the payload
pre-filter (ops/csrc/engine.inc) has work to skip. Same feeding as
``benchmarks/pipeline_micro.py`` (cache-hot reads of 4 MiB into
``Pipeline.feed_chunked``), one row per decode-thread count, and the payloads
decode built and left unbuilt from ``_kwcore.apply_stats()`` where the module
has them. One JSON line, for paired runs of two trees.

    python -m benchmarks.prefilter_micro [--pods 4000] [--threads 0,auto] [--reps 5] [--prefilter on|off]
"""

from __future__ import annotations

import argparse
import json
import sys
import time

from k8s_watcher_amd.ops.native import load
from k8s_watcher_amd.testing.podgen import NAMESPACES_DEFAULT
from k8s_watcher_amd.testing.replay_server import Template
from k8s_watcher_amd.utils.cpus import auto_decode_threads

READ_SIZE = 4 << 20


def ns_per_event(mod, data: bytes, n: int, threads: int, nsset, reps: int) -> float:
    chunks = [data[j:j + READ_SIZE] for j in range(0, len(data), READ_SIZE)]
    best = float("inf")
    for _ in range(reps):
        notifier = mod.Notifier(b"POST /x HTTP/1.1\r\nContent-Length: ", 4, 32, 3, 1.0, 2.0, 30.0,
                                False, False, [502, 503], {})
        pl = mod.Pipeline("production", mod.PodCache(), {}, nsset, True, False, 1, 0, True, True, notifier,
                          False, False, threads)
        spent = 0
        for ch in chunks:
            hot = bytearray(ch)  # like a recv buffer: just written, in cache
            t0 = time.perf_counter_ns()
            pl.feed_chunked(hot, 0)
            spent += time.perf_counter_ns() - t0
        best = min(best, spent)
        del pl, notifier
    return best / n


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pods", type=int, default=4000)
    ap.add_argument("--threads", default="0,auto")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prefilter", default="on", choices=["on", "off"])
    args = ap.parse_args(argv)
    mod = load()
    if hasattr(mod, "set_payload_prefilter"):
        mod.set_payload_prefilter(args.prefilter == "on")
    elif args.prefilter == "off":
        ap.error("this build has no payload pre-filter to turn off")
    t = Template("churn", args.pods, 0)
    data, offs = t.render(0, 0, len(t))
    n = len(offs)
    nsset = frozenset(NAMESPACES_DEFAULT[::2])  # half of the corpus's namespaces
    res = {"events": n, "bytes_per_event": round(len(data) / n), "namespaces_allowed": sorted(nsset),
           "prefilter": args.prefilter if hasattr(mod, "set_payload_prefilter") else None, "ns_per_event": {}}
    for spec in args.threads.split(","):
        threads = auto_decode_threads() if spec == "auto" else int(spec)
        before = mod.apply_stats()
        res["ns_per_event"]["%s(%d)" % (spec, threads) if spec == "auto" else spec] = round(
            ns_per_event(mod, data, n, threads, nsset, args.reps), 1)
        after = mod.apply_stats()
        if "payload_built" in after:
            res["payload_built_frac"] = round((after["payload_built"] - before["payload_built"]) / (n * args.reps), 4)
            res["payload_prefiltered_frac"] = round(
                (after["payload_prefiltered"] - before["payload_prefiltered"]) / (n * args.reps), 4)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

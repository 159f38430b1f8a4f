#!/usr/bin/env bash
# decode_line with the payload pre-filter (ops/csrc/engine.inc) under
# AddressSanitizer and UBSan — or ThreadSanitizer — as a stand-alone program on
# the CPU: ops/csrc/check/prefilter_check.cpp has its own main and never starts
# the interpreter. Four threads share one DecodeCfg and one namespace set, as
# the decode workers do, and decode the corpus of
# tests/test_payload_prefilter.py unsharded and as each of four shards, by
# namespace and by uid; what the program reports of every line is compared
# with what the test expects. watcher.alerts.terminating is on in the program:
# the corpus has the timestamp on DELETED lines only, so a second file of
# Running pods, every other one terminating, in allowed and other namespaces,
# goes through the same configurations — the program compares the signature
# on and off and with the pod's own, and exactly the terminating lines must
# be the ones the critical filter keeps.
#
#   scripts/prefilter_check.sh [address|thread]
set -euo pipefail
cd "$(dirname "$0")/.."
kind=${1:-address}
case "$kind" in
    address) san="-fsanitize=address,undefined -fno-sanitize-recover=all" ;;
    thread) san="-fsanitize=thread" ;;
    *) echo "usage: $0 [address|thread]" >&2; exit 2 ;;
esac
out=build/prefilter-check-$kind
mkdir -p "$out"
# shellcheck disable=SC2046
"${CXX:-g++}" -std=c++20 -O1 -g -fno-omit-frame-pointer $san -pthread -fno-strict-aliasing \
    -Wall -Wno-shadow -Wno-unused-function -Wno-psabi $(python3-config --includes) -Ik8s_watcher_amd/ops/csrc \
    k8s_watcher_amd/ops/csrc/check/prefilter_check.cpp -o "$out/prefilter_check" \
    $(python3-config --embed --ldflags) -lssl -lcrypto -lz
python3 - "$out" <<'EOF'
import subprocess
import sys

sys.path[:0] = [".", "tests"]
import test_payload_prefilter as t
import test_terminating_alerts as tt
from k8s_watcher_amd.testing.podgen import PodFactory, event_line

out = sys.argv[1]
warm, data, rows = t.corpus()
with open(f"{out}/lines.ndjson", "wb") as fh:
    fh.write(warm + data)
TIDX = {"ADDED": 0, "MODIFIED": 1, "DELETED": 2, "BOOKMARK": 3}
for shard in t.SHARDINGS:
    count, index, by_uid = (1, 0, 0) if shard is None else (t.SHARDS, shard[1], int(shard[0] == "uid"))
    res = subprocess.run([f"{out}/prefilter_check", f"{out}/lines.ndjson", str(count), str(index), str(by_uid),
                          *t.ALLOWED], capture_output=True, text=True)
    sys.stderr.write(res.stderr)
    if res.returncode:
        sys.exit(f"prefilter_check failed ({res.returncode}) for {shard}")
    got = [tuple(int(x) for x in ln.split()) for ln in res.stdout.splitlines()]
    assert [g[0] for g in got] == [TIDX[r[0]] for r in rows], shard
    built, pre = t.expected_payloads(rows, t.ALLOWED, shard)
    assert sum(g[1] for g in got) == pre and sum(g[2] for g in got) == built, (shard, built, pre)
    assert sum(g[3] for g in got) == built + pre, shard
    for g, r in zip(got, rows):
        assert (g[1] or g[2]) == (r[3] and r[0] != "BOOKMARK"), (shard, g, r)  # exactly the critical-kept lines
f = PodFactory(seed=5, namespaces=list(t.ALLOWED) + ["elsewhere", "batch-jobs"])
term, seen_built = [], False
for i in range(240):
    pod = f.running(f.new_pod())
    term.append(tt.deleting(pod, i + 1) if i % 2 else tt.with_rv(pod, i + 1))
with open(f"{out}/terminating.ndjson", "wb") as fh:
    fh.write(b"".join(event_line("ADDED" if i % 3 == 0 else "MODIFIED", pod) for i, pod in enumerate(term)))
for shard in t.SHARDINGS:
    count, index, by_uid = (1, 0, 0) if shard is None else (t.SHARDS, shard[1], int(shard[0] == "uid"))
    res = subprocess.run([f"{out}/prefilter_check", f"{out}/terminating.ndjson", str(count), str(index), str(by_uid),
                          *t.ALLOWED], capture_output=True, text=True)
    sys.stderr.write(res.stderr)
    if res.returncode:
        sys.exit(f"prefilter_check failed ({res.returncode}) for the terminating lines, {shard}")
    got = [tuple(int(x) for x in ln.split()) for ln in res.stdout.splitlines()]
    assert len(got) == len(term), shard
    for i, g in enumerate(got):
        assert bool(g[1] or g[2]) == bool(i % 2), (shard, i, g)  # kept by the critical filter: the terminating ones
        assert g[3] == i % 2, (shard, i, g)
    assert any(g[1] for g in got), shard  # the other namespaces' at least are pre-dropped
    seen_built = seen_built or any(g[2] for g in got)
assert seen_built
print(f"prefilter_check: {len(rows)} lines x {len(t.SHARDINGS)} configurations as expected, sanitizers silent")
EOF

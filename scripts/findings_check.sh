#!/usr/bin/env bash
# The container failure and pod condition findings walkers, the terminating
# finding, the deletion deadline, the pending-since and the unready-since (ops/csrc/findings.inc over scanner.inc) under AddressSanitizer and
# UBSan, as a stand-alone program on the CPU — no Python in the process. It
# walks the corpora of tests/test_container_failures.py,
# tests/test_pod_condition_alerts.py, tests/test_terminating_alerts.py, the
# timestamp corpus of tests/test_termination_overdue.py and the corpora of
# tests/test_pending_overdue.py and tests/test_unready_overdue.py
# (each pod through the filter-first and the full parse, with every scanner
# form the CPU has), compares the three kinds of findings and the JSON of the
# extra field termination with the expected ones and every pod's deletion
# deadline, pending-since and unready-since with models/findings.py
# deletion_deadline, pending_since and unready_since, then walks MUTATIONS
# (default 200) mutated copies of every pod and of the fuzz pods of the
# condition, terminating, overdue, pending and unready tests.
#
#   scripts/findings_check.sh [MUTATIONS]
set -euo pipefail
cd "$(dirname "$0")/.."
out=build/findings-check
mkdir -p "$out"
"${CXX:-g++}" -std=c++20 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Wall -Wno-unused-function k8s_watcher_amd/ops/csrc/check/findings_check.cpp -o "$out/findings_check"
python3 - "$out" "${1:-200}" <<'EOF'
import json
import subprocess
import sys

sys.path[:0] = [".", "tests"]
import test_container_failures as t
import test_pod_condition_alerts as tc
import test_terminating_alerts as tt
import test_termination_overdue as to
import test_pending_overdue as tp
import test_unready_overdue as tu
from k8s_watcher_amd.models.findings import (condition_findings, container_findings, deletion_deadline, pending_since,
                                             terminating, unready_since)

out, mutations = sys.argv[1], sys.argv[2]
pods = [t.corpus_pod(init_raw, cs_raw) for _, init_raw, cs_raw, _ in t.CORPUS]
pods += [tc.corpus_pod(status_raw) for _, status_raw, _ in tc.CORPUS]
pods += [json.dumps(json.loads(ln)["object"], separators=(",", ":")) for ln in tc.fuzz_lines(100)]
n_before = len(pods)
pods += [tt.corpus_object(members) for _, members, _, _ in tt.CORPUS]  # raw: repeated and escaped keys as written
pods += [ln[ln.index(b'"object":') + 9:-2].decode() for ln in tt.fuzz_lines(200)]
n_stamps = len(pods)
stamps = to.timestamp_corpus()
pods += [pod for pod, _ in stamps]
pods += to.fuzz_pods(200)
n_pending = len(pods)
pending = tp.corpus_pods()
pods += [pod for pod, _ in pending]
pods += tp.fuzz_pods(200)
n_unready = len(pods)
unready = tu.corpus_pods()
pods += [pod for pod, _ in unready]
pods += tu.fuzz_pods(200)
with open(f"{out}/pods.jsonl", "w") as fh:
    for pod in pods:
        fh.write(pod + "\n")
res = subprocess.run([f"{out}/findings_check", f"{out}/pods.jsonl", mutations], capture_output=True, text=True)
sys.stderr.write(res.stderr)
if res.returncode:
    sys.exit(f"findings_check failed ({res.returncode})")
rows = [ln.split("\t") for ln in res.stdout.splitlines()]
assert len(rows) == len(pods), (len(rows), len(pods))
for pod, (sig, found, cond_sig, conds, term_sig, term, due, since, bad) in zip(pods, rows):
    obj = json.loads(pod)
    for want, got, s in ((container_findings(obj), found, sig), (condition_findings(obj), conds, cond_sig)):
        assert json.loads(got) == want, (pod, got, want)
        assert (int(s) == 0) == (not want), (pod, s)
    assert int(term_sig) == int(terminating(obj)), (pod, term_sig)
    assert json.loads(term) == tt.want_termination(obj), (pod, term)
    assert (None if due == "-" else int(due)) == deletion_deadline(obj), (pod, due)
    assert (None if since == "-" else int(since)) == pending_since(obj), (pod, since)
    assert (None if bad == "-" else int(bad)) == unready_since(obj), (pod, bad)
for (name, _, _, want), (_, found, *_) in zip(t.CORPUS, rows):
    assert json.loads(found) == want, (name, found, want)
for (name, _, want), (_, _, _, conds, *_) in zip(tc.CORPUS, rows[len(t.CORPUS):]):
    assert json.loads(conds) == want, (name, conds, want)
for (name, _, _, want), (*_, term_sig, _, _, _, _) in zip(tt.CORPUS, rows[n_before:]):
    assert int(term_sig) == int(want), (name, term_sig, want)
for (pod, want), (*_, due, _, _) in zip(stamps, rows[n_stamps:]):
    assert (None if due == "-" else int(due)) == want, (pod, due, want)
assert sum(r[-3] != "-" for r in rows[n_stamps + len(stamps):n_pending]) >= 30  # the fuzz pods have deadlines too
for (pod, want), (*_, since, _) in zip(pending, rows[n_pending:]):
    assert (None if since == "-" else int(since)) == want, (pod, since, want)
fuzz_since = [r[-2] != "-" for r in rows[n_pending + len(pending):n_unready]]
assert sum(fuzz_since) >= 20 and fuzz_since.count(False) >= 20  # ... and pending-sinces, and none
for (pod, want), (*_, bad) in zip(unready, rows[n_unready:]):
    assert (None if bad == "-" else int(bad)) == want, (pod, bad, want)
fuzz_bad = [r[-1] != "-" for r in rows[n_unready + len(unready):]]
assert sum(fuzz_bad) >= 20 and fuzz_bad.count(False) >= 20  # ... and unready-sinces, and none
print(f"findings_check: {len(rows)} pods as expected ({len(t.CORPUS)} + {len(tc.CORPUS)} + {len(tt.CORPUS)} + "
      f"{len(stamps)} + {len(pending)} + {len(unready)} corpus), deadline, pending-since and unready-since columns "
      "checked, sanitizers silent")
EOF

#!/usr/bin/env bash
# The container failure findings walker (ops/csrc/findings.inc over scanner.inc)
# under AddressSanitizer and UBSan, as a stand-alone program on the CPU — no
# Python in the process. It walks the corpus of tests/test_container_failures.py
# (each pod through the filter-first and the full parse, with every scanner
# form the CPU has), compares the findings with the expected ones, then walks
# MUTATIONS (default 200) mutated copies of every pod.
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

out, mutations = sys.argv[1], sys.argv[2]
with open(f"{out}/pods.jsonl", "w") as fh:
    for _, init_raw, cs_raw, _ in t.CORPUS:
        fh.write(t.corpus_pod(init_raw, cs_raw) + "\n")
res = subprocess.run([f"{out}/findings_check", f"{out}/pods.jsonl", mutations], capture_output=True, text=True)
sys.stderr.write(res.stderr)
if res.returncode:
    sys.exit(f"findings_check failed ({res.returncode})")
rows = [ln.split("\t", 1) for ln in res.stdout.splitlines()]
assert len(rows) == len(t.CORPUS), (len(rows), len(t.CORPUS))
for (name, _, _, want), (sig, found) in zip(t.CORPUS, rows):
    assert json.loads(found) == want, (name, found, want)
    assert (int(sig) == 0) == (not want), (name, sig)
print(f"findings_check: {len(rows)} corpus pods as expected, sanitizers silent")
EOF

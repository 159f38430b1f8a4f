#!/usr/bin/env bash
# The chunked-body framer and NDJSON line splitter (ops/csrc/chunked.inc) under
# AddressSanitizer and UBSan, as a stand-alone program on the CPU — no Python
# in the process. It frames the valid framings and the framing errors of
# tests/test_chunk_framing.py whole, at every two-piece cut and one byte at a
# time, the string-carrying consumers' way and the reader hub's, and compares
# the recovered lines, the final state and the error texts with the test's
# expected values.
#
#   scripts/chunked_check.sh
set -euo pipefail
cd "$(dirname "$0")/.."
out=build/chunked-check
mkdir -p "$out"
"${CXX:-g++}" -std=c++20 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Wall -Wno-unused-function k8s_watcher_amd/ops/csrc/check/chunked_check.cpp -o "$out/chunked_check"
python3 - "$out" <<'PY'
import subprocess
import sys

sys.path[:0] = [".", "tests"]
import test_chunk_framing as t

out = sys.argv[1]
rows = [(name, raw, t.LINES, "done" if done else "state 0 remain 0 open 0") for name, (raw, done) in t.FRAMINGS.items()]
rows += [(name, valid + bad + after, t.LINES[:t.N_BEFORE], "error " + text.encode().hex())
         for name, (valid, bad, after, text) in t.ERRORS.items()]
with open(f"{out}/framings.tsv", "w") as fh:
    for name, raw, _lines, _end in rows:
        fh.write(f"{name}\t{raw.hex()}\n")
res = subprocess.run([f"{out}/chunked_check", f"{out}/framings.tsv"], capture_output=True, text=True)
sys.stderr.write(res.stderr)
if res.returncode:
    sys.exit(f"chunked_check failed ({res.returncode})")
got = [ln.split("\t") for ln in res.stdout.splitlines()]
assert len(got) == len(rows), (len(got), len(rows))
for (name, _raw, lines, end), (gname, gend, *glines) in zip(rows, got):
    assert gname == name and gend == end, (name, gend, end)
    assert [bytes.fromhex(x) for x in glines] == lines, (name, glines)
print(f"chunked_check: {len(t.FRAMINGS)} framings and {len(t.ERRORS)} framing errors as expected, sanitizers silent")
PY

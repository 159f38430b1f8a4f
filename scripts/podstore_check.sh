#!/usr/bin/env bash
# The pod cache's store (ops/csrc/podstore.inc: the per-namespace and
# per-timer-kind intrusive lists, the overdue take, the whole-entry replace)
# under AddressSanitizer and UBSan, as a stand-alone program on the CPU — no
# Python in the process. A seeded random operation sequence of STEPS steps
# (default 5000) is checked against a std::map model after every step
# (ops/csrc/check/podstore_check.cpp), with a second seed for good measure.
#
#   scripts/podstore_check.sh [STEPS]
set -euo pipefail
cd "$(dirname "$0")/.."
out=build/podstore-check
mkdir -p "$out"
"${CXX:-g++}" -std=c++20 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Wall -Wno-unused-function k8s_watcher_amd/ops/csrc/check/podstore_check.cpp -o "$out/podstore_check"
"$out/podstore_check" "${1:-5000}"
"$out/podstore_check" "${1:-5000}" 7
echo "podstore_check: the store agrees with its model, sanitizers silent"

#!/usr/bin/env bash
# Builds oracle/_ref/libphm_ref.so: the reference's own src/phylomap.cpp, compiled in place from the reference tree against the
# stand-in Rcpp / RcppArmadillo headers of oracle/ref/stub/, together with oracle/ref/ref_entry.cpp (C entry points) and a private
# copy of the oracle (the R-stream generators the stand-in forwards to).  TEST INFRASTRUCTURE for tests/test_reference_pin_cpu.py.
#
# The reference tree is read where PHM_REFERENCE_DIR points (default /root/reference); nothing of it is copied, and the output
# directory is ignored by git.  Without the tree this script does nothing and succeeds.  A compile error is passed on with the
# compiler's message.  Floating point as for the oracle: no contraction, no fast-math, no -march=native.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ref="${PHM_REFERENCE_DIR:-/root/reference}"
if [ ! -f "$ref/src/phylomap.cpp" ]; then
  echo "ref_build: no reference tree at $ref, nothing to do"
  exit 0
fi
out="${PHM_REF_OUT:-$here/_ref}"
mkdir -p "$out"
fpflags="-O2 -fPIC -ffp-contract=off -fno-fast-math"
fma=""
if grep -q -w fma /proc/cpuinfo 2>/dev/null; then fma="-mfma"; fi     # as oracle/Makefile: explicit fma() calls only
extra="${PHM_REF_EXTRA_FLAGS:-}"                                       # e.g. "-fsanitize=address,undefined -g" for a host-side check
# two compile jobs side by side, then the link
"${CC:-gcc}" $fpflags $fma $extra -std=c11 -c "$here/phm_oracle.c" -o "$out/phm_oracle.o" &
cpid=$!
"${CXX:-g++}" $fpflags $extra -std=c++17 -w -I "$here/ref/stub" -I "$ref/src" -c "$here/ref/ref_entry.cpp" -o "$out/ref_entry.o"
wait "$cpid"
"${CXX:-g++}" -shared $extra -Wl,-Bsymbolic -o "$out/libphm_ref.so" "$out/ref_entry.o" "$out/phm_oracle.o" -lm
echo "ref_build: $out/libphm_ref.so"

#!/bin/sh
# Build tools/tx_copy_check.cpp for the CPU under AddressSanitizer and UBSan and run it: the copy of
# shorthair_tx_datagram_batch on exact-size heap buffers. No GPU. CXX must be a clang++ (vector extensions).
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-clang++} -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    -o "$out/tx_copy_check" "$here/tx_copy_check.cpp"
"$out/tx_copy_check"

#!/bin/sh
# Build tools/rx_window_copy_check.cpp for the CPU under AddressSanitizer and UBSan and run it: the copy of
# shorthair_rx_window_batch on exact-size heap buffers. No GPU. CXX must be a clang++ (vector extensions).
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-clang++} -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    -o "$out/rx_window_copy_check" "$here/rx_window_copy_check.cpp"
"$out/rx_window_copy_check"

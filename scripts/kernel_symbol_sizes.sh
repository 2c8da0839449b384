#!/bin/bash
# Size and name of every kernel in the gfx950 code object embedded in a HIP object file, plus a hash of the code object:
#     scripts/kernel_symbol_sizes.sh robustvlm_amd/csrc/build/attention_bf16.o
# Two builds of a translation unit compiled to the same code exactly when the outputs are equal - the check that a change
# beside the image path (a new translation unit, a header addition) left the shipped kernels alone.
set -e
B=${ROCM_PATH:-/opt/rocm}/llvm/bin
t=$(mktemp -d)
trap 'rm -rf "$t"' EXIT
"$B/llvm-objcopy" --dump-section .hip_fatbin="$t/fat.bin" "$1"
"$B/clang-offload-bundler" --unbundle --type=o --input="$t/fat.bin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$t/k.co"
"$B/llvm-readelf" -s --wide "$t/k.co" | awk '$4 == "FUNC" {print $3, $8}' | sort -k2
sha256sum < "$t/k.co" | cut -c1-16 | sed 's/^/code-object-sha256 /'

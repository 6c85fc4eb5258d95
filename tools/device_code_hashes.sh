#!/bin/bash
# Developer tool: SHA-256 of the gfx950 code object inside every object file of a built tree -- two builds with equal hashes run the
# same device code, whatever their host code does ("-" for an object without device code).
#   tools/device_code_hashes.sh [obia_amd/csrc]
dir=$(realpath "${1:-$(dirname "$0")/../obia_amd/csrc}")
LLVM=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
for o in "$dir"/*.o; do
  tmp=$(mktemp -d); cp "$o" $tmp/in.o; (cd $tmp && $LLVM/llvm-objdump --offloading in.o >/dev/null 2>&1)
  co=$(ls $tmp/*amdgcn* 2>/dev/null | head -1)
  printf "%-16s %s\n" "$(basename "$o")" "$([ -n "$co" ] && sha256sum "$co" | cut -d' ' -f1 || echo -)"
  rm -rf $tmp
done

#!/bin/bash
# Developer tool: SHA-256 of the gfx950 code object inside every object file of a built tree -- two builds with equal hashes run the
# same device code, whatever their host code does ("-" for an object without device code).
#   tools/device_code_hashes.sh [obia_amd/csrc]
# Host code that instantiates the same kernels in another order moves them around inside the code object and changes that hash.
# --kernels: a SHA-256 of every kernel's own bytes in .text instead (the symbols that have a kernel descriptor NAME.kd), sorted by
# name -- equal listings mean the same kernels, byte for byte, wherever they lie.
#   tools/device_code_hashes.sh --kernels [obia_amd/csrc]
kernels=0
if [ "$1" = "--kernels" ]; then kernels=1; shift; fi
dir=$(realpath "${1:-$(dirname "$0")/../obia_amd/csrc}")
LLVM=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
for o in "$dir"/*.o; do
  tmp=$(mktemp -d); cp "$o" $tmp/in.o; (cd $tmp && $LLVM/llvm-objdump --offloading in.o >/dev/null 2>&1)
  co=$(ls $tmp/*amdgcn* 2>/dev/null | head -1)
  if [ $kernels = 0 ]; then
    printf "%-16s %s\n" "$(basename "$o")" "$([ -n "$co" ] && sha256sum "$co" | cut -d' ' -f1 || echo -)"
  elif [ -n "$co" ]; then
    { $LLVM/llvm-readelf -S -W "$co"; $LLVM/llvm-readelf --symbols -W "$co"; } | python3 -c '
import hashlib, re, sys
obj, path = sys.argv[1], sys.argv[2]
text, syms = None, {}
for ln in sys.stdin:
    m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
    if m: text = [int(x, 16) for x in m.groups()]   # address, file offset, size
    m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+\S+\s+(\S+)", ln)
    if m: syms[m.group(4)] = (int(m.group(1), 16), int(m.group(2)), m.group(3))
data = open(path, "rb").read()
for name in sorted(n for n in syms if syms[n][2] == "FUNC" and n + ".kd" in syms):
    addr, size, _ = syms[name]
    off = text[1] + addr - text[0]
    print("%-24s %s %6d %s" % (obj, hashlib.sha256(data[off:off + size]).hexdigest(), size, name))
' "$(basename "$o")" "$co"
  fi
  rm -rf $tmp
done

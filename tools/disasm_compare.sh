#!/bin/bash
# usage: tools/disasm_compare.sh OLD_OBJ_DIR NEW_OBJ_DIR
# Diffs the gfx950 disassembly (llvm-objdump -d of the code object in each unit's .hip_fatbin) of every object of two builds
# that carries device code (e.g. a copy of degnorm_amd/csrc/obj from the parent commit and the current one); objects without a
# .hip_fatbin section are skipped.  Prints "DIFF: <unit>" per unit that changed and the number compared; exit status 1 if any
# changed.  No GPU needed.
set -u
B=${ROCM_PATH:-/opt/rocm}/llvm/bin
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
rc=0; n=0
for o in "$1"/*.o; do
  f=$(basename "$o")
  "$B/llvm-objdump" --section-headers "$o" | grep -q '\.hip_fatbin' || continue
  for side in old new; do
    src=$([ $side = old ] && echo "$1/$f" || echo "$2/$f")
    "$B/llvm-objcopy" --dump-section=.hip_fatbin="$W/$side.fatbin" "$src" &&
    "$B/clang-offload-bundler" --unbundle --type=o --input="$W/$side.fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
        --output="$W/$side.co" &&
    "$B/llvm-objdump" -d --no-show-raw-insn "$W/$side.co" | tail -n +3 > "$W/$side.dis" || { echo "FAILED: $f ($side)"; rc=1; }
  done
  if ! cmp -s "$W/old.dis" "$W/new.dis"; then echo "DIFF: $f"; rc=1; fi
  n=$((n + 1))
done
echo "compared $n units"
exit $rc

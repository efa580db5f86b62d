#!/usr/bin/env bash
# Device code of the working tree against a git revision (default HEAD): for every translation unit of csrc/Makefile's SRCS
# the gfx950 assembly is emitted with the Makefile's flags plus --offload-device-only -S on both trees and diffed.  A change
# that is meant to touch host code only prints "identical" ten times and exits 0.  No GPU needed; takes a few minutes.
# (The one symbol clang names after a hash of the whole source text, __hip_cuid_<hash>, is written without its hash.)
#   bash profiles/device_code_diff.sh [revision]
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
rev=${1:-HEAD}
csrc=denseslam-global-consistency-h_amd/csrc
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/base" "$tmp/asm"
git -C "$root" archive "$rev" "$csrc" include | tar -x -C "$tmp/base"
srcs=$(make -s -C "$root/$csrc" --eval='print-srcs: ; @echo $(SRCS)' print-srcs)
flags=$(make -s -C "$root/$csrc" --eval='print-flags: ; @echo $(HIPCC) $(HIPFLAGS)' print-flags)
flags="$flags -Wno-unused-command-line-argument"
status=0
for src in $srcs; do
  (cd "$tmp/base/$csrc" && $flags --offload-device-only -S "$src" -o "$tmp/asm/${src%.hip}.base.s") &
  (cd "$root/$csrc" && $flags --offload-device-only -S "$src" -o "$tmp/asm/${src%.hip}.new.s") &
  wait
  sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s"
  if diff -q "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s" >/dev/null; then
    echo "$src: identical ($(wc -l < "$tmp/asm/${src%.hip}.new.s") lines)"
  else
    echo "$src: DIFFERS"
    diff "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s" | head -20 || true
    status=1
  fi
done
exit $status

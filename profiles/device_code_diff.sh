#!/usr/bin/env bash
# Device code of the working tree against a git revision (default HEAD): for every translation unit of csrc/Makefile's SRCS
# the gfx950 assembly is emitted with the Makefile's flags plus --offload-device-only -S on both trees and diffed.  A change
# that is meant to touch host code only prints "identical" ten times and exits 0.  No GPU needed; takes a few minutes.
# (The one symbol clang names after a hash of the whole source text, __hip_cuid_<hash>, is written without its hash.)
#   bash profiles/device_code_diff.sh [--resources] [revision]
# --resources: for a unit that differs, also the per-kernel resources the compiler reports in the assembly's metadata, revision
# against tree (VGPRs, SGPR / VGPR spills, scratch and LDS bytes, occupancy in waves per SIMD); kernels that differ are marked.
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
resources=0
if [ "${1:-}" = "--resources" ]; then resources=1; shift; fi
rev=${1:-HEAD}
# kernel -> "vgprs sgpr_spills vgpr_spills scratch lds occupancy" from the .amdhsa_kernel blocks, the occupancy note and the metadata
kernel_resources() {
  awk '$1 == ".amdhsa_kernel" { k = $2 }
       $1 == ";" && $2 == "Occupancy:" { occ[k] = $3 }
       $1 == ".group_segment_fixed_size:" { lds = $2 }
       $1 == ".name:" { n = $2 }
       $1 == ".private_segment_fixed_size:" { scr = $2 }
       $1 == ".sgpr_spill_count:" { ss = $2 }
       $1 == ".vgpr_count:" { vg = $2 }
       $1 == ".vgpr_spill_count:" { print n, vg, ss, $2, scr, lds, occ[n] }' "$1" | sort
}
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
  if [ ! -f "$tmp/base/$csrc/$src" ]; then echo "$src: new in the tree (not in $rev)"; continue; fi
  (cd "$tmp/base/$csrc" && $flags --offload-device-only -S "$src" -o "$tmp/asm/${src%.hip}.base.s") &
  (cd "$root/$csrc" && $flags --offload-device-only -S "$src" -o "$tmp/asm/${src%.hip}.new.s") &
  wait
  sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s"
  if diff -q "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s" >/dev/null; then
    echo "$src: identical ($(wc -l < "$tmp/asm/${src%.hip}.new.s") lines)"
  else
    echo "$src: DIFFERS"
    diff "$tmp/asm/${src%.hip}.base.s" "$tmp/asm/${src%.hip}.new.s" | head -20 || true
    if [ $resources = 1 ]; then
      echo "kernel | vgprs sgpr_spills vgpr_spills scratch lds occupancy: $rev | tree"
      join -a1 -a2 -e - -o 0,1.2,1.3,1.4,1.5,1.6,1.7,2.2,2.3,2.4,2.5,2.6,2.7 <(kernel_resources "$tmp/asm/${src%.hip}.base.s") \
        <(kernel_resources "$tmp/asm/${src%.hip}.new.s") |
        awk '{ m = ($2 == $8 && $3 == $9 && $4 == $10 && $5 == $11 && $6 == $12 && $7 == $13) ? " " : "*"
               print m, $1, "|", $2, $3, $4, $5, $6, $7, "|", $8, $9, $10, $11, $12, $13 }' | { c++filt 2>/dev/null || cat; }
    fi
    status=1
  fi
done
exit $status

#!/bin/bash
# Is the device code of this tree the device code of another checkout?  (No GPU needed; the proof that a change which only moves
# definitions between headers moved nothing else.)
#   bash tools/device_asm_same.sh /path/to/other/checkout
# Each of the four units is compiled in both trees, from the same relative path, with the Makefile's HIPFLAGS plus
# --offload-device-only -S (one tree after the other, a tree's four units side by side); the one symbol the compiler derives from the
# source's path and text (__hip_cuid_<hash>) is replaced by a fixed word, and the two files are compared whole with cmp.
# Exit status 0: all four identical, byte for byte.  Otherwise the assembly and the compilers' messages are kept and their place is printed.
set -u -o pipefail
here="$(cd "$(dirname "$0")/.." && pwd)"
other="$(cd "${1:?the other checkout}" && pwd)"
out="$(mktemp -d)"
flags() { sed -n 's/^HIPFLAGS ?= //p' "$1/portcullis_amd/csrc/Makefile" | sed "s/\$(ARCH)/$(sed -n 's/^ARCH ?= //p' "$1/portcullis_amd/csrc/Makefile")/"; }
units="pjb_api pjb_extra_api pjb_model_api pjb_ingest_api"
for side in here other; do
  tree="${!side}"
  mkdir -p "$out/$side"
  for u in $units; do
    (cd "$tree/portcullis_amd/csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} $(flags "$tree") --offload-device-only -S -o "$out/$side/$u.raw.s" "$u.hip" 2> "$out/$side/$u.err") &
  done
  wait
done
status=0
echo "flags: $(flags "$here") --offload-device-only -S"
for u in $units; do
  for side in here other; do
    [ -s "$out/$side/$u.raw.s" ] || { echo "$u: did not compile in ${!side}"; status=1; continue 2; }
    sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out/$side/$u.raw.s" > "$out/$side/$u.s"
  done
  kernels="$(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$out/here/$u.s") / $(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$out/other/$u.s")"
  lines="$(wc -l < "$out/here/$u.s") / $(wc -l < "$out/other/$u.s")"
  if cmp -s "$out/here/$u.s" "$out/other/$u.s"; then verdict="identical"; else verdict="DIFFERENT ($(cmp "$out/here/$u.s" "$out/other/$u.s" 2>&1 | head -1))"; status=1; fi
  printf '%-16s kernels %s, lines %s: %s\n' "$u" "$kernels" "$lines" "$verdict"
done
if [ $status -eq 0 ]; then rm -rf "$out"; else echo "kept for a look: $out"; fi
exit $status

#!/bin/bash
# print "sha256  file" of the DEVICE code object of every translation unit of the product library: build.py's SOURCES compiled
# with build.py's FLAGS plus -fuse-cuid=none --cuda-device-only (without -fuse-cuid=none two compiles of one source differ in
# a random per-unit id).  A refactor of csrc/ that is meant to change no kernel gives the same listing before and after; the
# listing of an older commit is  git worktree add <dir> <commit> && <dir>/tools/device_code_digest.sh  (or this script copied
# into that tree).  Reads nothing outside the tree, needs no GPU.
set -euo pipefail
cd "$(dirname "$0")/../ddsp_svc_amd"
W=$(mktemp -d); trap 'rm -rf "$W"' EXIT
# (build.py on its own: importing the package would load the library)
read -r HIPCC FLAGS < <(python3 -c "import build as b; print(b._hipcc(), *b.FLAGS)")
for src in $(python3 -c "import build as b; print(*b.SOURCES)"); do
  "$HIPCC" $FLAGS -fuse-cuid=none --cuda-device-only -c "csrc/$src" -o "$W/$src.o"
  printf '%s  %s\n' "$(sha256sum "$W/$src.o" | cut -d' ' -f1)" "$src"
done

#!/bin/bash
# Compare the gfx950 device code of every kernel file with that of a parent revision, for refactors that must not change it:
#   tools/kernel_diff.sh REV ["-DEXTRA=1 ..."] [file.hip ...]      (default: every .hip file under csrc/)
# Both trees are compiled from the same relative path with the Makefile's HIPFLAGS plus --cuda-device-only -S.  Mangled
# names and the per-unit __hip_cuid_ symbol are masked, then the listings must be equal line for line: every instruction
# of every instantiation and every kernel's register, spill, scratch and LDS figures.  A file whose listing is equal even
# unmasked (it includes nothing that changed) has its object compared byte for byte as well.
# One row per file: file | kernels | lines | result.  Exit status 1 if any file differs.  Listings stay in $OUT
# (default a fresh temporary directory); JOBS compilations run at a time (default 8).
set -e -o pipefail
REV=${1:?usage: kernel_diff.sh REV [flags] [files]}; FLAGS=$2; shift; [ $# -gt 0 ] && shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SUB=directx-raytracer_amd/csrc
OUT=${OUT:-$(mktemp -d)}
HIPFLAGS="-std=c++17 -O3 -fPIC -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -Wall -Wextra" # csrc/Makefile
mkdir -p "$OUT/old" "$OUT/new/$SUB"
git -C "$ROOT" archive "$REV" "$SUB" include | tar -x -C "$OUT/old"
mkdir -p "$OUT/new/include" && cp "$ROOT"/include/*.h "$OUT/new/include/" && cp "$ROOT/$SUB"/*.h "$ROOT/$SUB"/*.hip "$OUT/new/$SUB/"
FILES=${*:-$(cd "$ROOT/$SUB" && ls *.hip)}
one() { # tree file: the masked listing, the plain one and the object
    cd "$OUT/$1/$SUB"
    if [ "$1" = old ] && [ -s "$2.masked.s" ]; then return; fi # a kept $OUT: the parent is compiled once per set of flags
    /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS --cuda-device-only -S "$2" -o "$2.s" 2> "$2.log"
    sed -E 's/_Z[A-Za-z0-9_.$]+/_Z/g; s/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$2.s" > "$2.masked.s"
}
export -f one; export OUT SUB HIPFLAGS FLAGS
for f in $FILES; do echo old $f; echo new $f; done | xargs -P "${JOBS:-8}" -n 2 bash -c 'one "$0" "$1"'
status=0
echo "file | kernels | lines | result"
for f in $FILES; do
    o=$OUT/old/$SUB/$f; n=$OUT/new/$SUB/$f
    kernels=$(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$n.s" || true); lines=$(wc -l < "$n.masked.s")
    if ! cmp -s "$o.masked.s" "$n.masked.s"; then
        res="DIFFERENT ($(diff "$o.masked.s" "$n.masked.s" | grep -c '^[<>]' || true) lines)"; status=1
    elif cmp -s "$o.s" "$n.s"; then
        for t in old new; do (cd "$OUT/$t/$SUB" && /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -c "$f" -o "$f.o" 2> /dev/null); done
        if cmp -s "$o.o" "$n.o"; then res="identical, object byte for byte"; else res="identical listing, OBJECT DIFFERS"; status=1; fi
    else
        res="identical"
    fi
    echo "$f | $kernels | $lines | $res"
done
echo "listings in $OUT"
exit $status

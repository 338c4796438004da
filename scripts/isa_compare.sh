#!/usr/bin/env bash
# Same machine code?  Compiles the device side of every source in csrc/build.sh's SRCS to gfx950 assembly, with
# build.sh's flags, in two trees and compares the texts with the per-translation-unit __hip_cuid_<hash> symbol masked.
# Both sides get the same -cuid=, which pins that hash and nothing else.  Everything up to the first data object (the
# kernels, their descriptors' inputs) must match line for line.  Behind it the compiler lays out a file's __device__
# variables in an order that is not stable from run to run (tron_conv_ws_pool.hip's g_ws_zero / g_ws_dump swap places
# between two compiles of the SAME source), so that tail is compared as a sorted set of lines.
# One line per source: identical or DIFFERENT.  Exit status 1 if any source differs or fails to compile.
#
#   scripts/isa_compare.sh <parent tree> <changed tree> [work dir]
#
# e.g.  git worktree add /tmp/parent HEAD~1 && scripts/isa_compare.sh /tmp/parent . > profiles/rNN_isa.txt
# The assembly is kept in <work dir>/{a,b}/<source>.s (default: a fresh temporary directory) for diffing by hand.
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 <parent tree> <changed tree> [work dir]" >&2; exit 2; }
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd)
WORK=${3:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC=deep-q-learning_tron_amd/csrc
# the flags and the source list are read from the changed tree's build.sh, so this cannot drift from the build
FLAGS=$(sed -n 's/^FLAGS="\(.*\)"$/\1/p' "$B/$CSRC/build.sh")
SRCS=$(sed -n 's/^SRCS="\(.*\)"$/\1/p' "$B/$CSRC/build.sh")
[ -n "$FLAGS" ] && [ -n "$SRCS" ] || { echo "cannot read FLAGS / SRCS from build.sh" >&2; exit 2; }
JOBS=${JOBS:-8}

mkdir -p "$WORK/a" "$WORK/b"
compile() {  # tree, out dir, source
    (cd "$1/$CSRC" && "$HIPCC" $FLAGS -cuid=isa_compare --cuda-device-only -S "$3" -o "$2/${3%.hip}.s") 2> "$2/${3%.hip}.err" || echo failed > "$2/${3%.hip}.failed"
}
n=0
for s in $SRCS; do
    rm -f "$WORK/a/${s%.hip}.failed" "$WORK/b/${s%.hip}.failed"
    [ -n "${SKIP_PARENT:-}" ] && [ -f "$WORK/a/${s%.hip}.s" ] || { compile "$A" "$WORK/a" "$s" & n=$((n + 1)); }
    compile "$B" "$WORK/b" "$s" & n=$((n + 1))
    if [ $n -ge "$JOBS" ]; then wait; n=0; fi
done
wait

# the code verbatim, then the data objects' lines sorted
norm() {
    sed 's/__hip_cuid_[0-9a-f]*/__hip_cuid_X/g' "$1" | awk '/,@object/ { tail = 1 } { if (tail) print | "sort"; else print }'
}
status=0
for s in $SRCS; do
    b=${s%.hip}
    if [ -f "$WORK/a/$b.failed" ] || [ -f "$WORK/b/$b.failed" ]; then
        echo "$s: COMPILE FAILED"; status=1
    elif cmp -s <(norm "$WORK/a/$b.s") <(norm "$WORK/b/$b.s"); then
        echo "$s: identical ($(wc -l < "$WORK/b/$b.s") lines of assembly)"
    else
        echo "$s: DIFFERENT"; status=1
    fi
done
exit $status

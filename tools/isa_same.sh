#!/bin/bash
# Is the gfx950 device code of this tree the same as that of another checkout (say, the parent commit
# in a git worktree)?  Builds, in both trees, the library's device assembly (make isa) and the
# scene-specialised kernels of five scenes (tools/jit_isa.sh: as is, the topology kernel, and the
# showcase's runtime sample/bounce loops), drops the lines holding the __hip_cuid_ symbol (a hash of the
# source text) and diffs the rest as plain text.  No GPU needed.  Exit status 0 = no differing line and
# equal resource lines (VGPRs, SGPRs, scratch, occupancy).
# usage: tools/isa_same.sh <other-tree>     (output: $ISA_OUT, default build/isa_same, in this tree)
set -o pipefail
OTHER=$(cd "${1:?other tree}" && pwd) || exit 2
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ISA_OUT:-$HERE/build/isa_same}
SCENES="sdf-showcase basic-demo advanced-demo deformation-stress mesh-demo"
mkdir -p "$OUT/this" "$OUT/other"

emit() {  # <tree> <dir>: the library's assembly, then every specialised kernel with its resource line
    local tree=$1 dir=$2 s
    make -C "$tree/rrte_amd/csrc" all isa > "$dir/make.log" 2>&1 || return 1
    for s in $(make -s -C "$tree/rrte_amd/csrc" print-src 2>/dev/null || echo rrte_hip.hip mesh_refit.hip mesh_build.hip); do  # one per unit (a tree from before print-src: its three)
        cp "$tree/build/isa/${s%.hip}.s" "$dir/" || return 1
    done
    : > "$dir/resources.txt"
    for s in $SCENES; do
        echo "$s full: $(cd "$tree" && bash tools/jit_isa.sh $s "$dir/jit_$s.s" | sed -n '1s/ \[-Rpass[^]]*\]//gp')" >> "$dir/resources.txt" || return 1
        echo "$s topo: $(cd "$tree" && RRTE_JIT_TOPO=1 bash tools/jit_isa.sh $s "$dir/jit_${s}_topo.s" | sed -n '1s/ \[-Rpass[^]]*\]//gp')" >> "$dir/resources.txt" || return 1
    done
    echo "sdf-showcase multi: $(cd "$tree" && RRTE_JIT_CHECK_MULTI=1 bash tools/jit_isa.sh sdf-showcase "$dir/jit_sdf-showcase_multi.s" | sed -n '1s/ \[-Rpass[^]]*\]//gp')" >> "$dir/resources.txt"
}
emit "$HERE" "$OUT/this" & P1=$!
emit "$OTHER" "$OUT/other" & P2=$!
wait $P1; R1=$?
wait $P2; R2=$?
[ $R1 = 0 ] || { echo "build failed in $HERE (see $OUT/this/make.log)"; exit 2; }
[ $R2 = 0 ] || { echo "build failed in $OTHER (see $OUT/other/make.log)"; exit 2; }

rc=0
for f in "$OUT"/this/*.s; do
    n=$(basename "$f")
    [ -s "$f" ] && [ -s "$OUT/other/$n" ] || { echo "MISSING $n"; rc=1; continue; }
    d=$(diff <(grep -v __hip_cuid_ "$OUT/other/$n") <(grep -v __hip_cuid_ "$f") | grep -c '^[<>]')
    printf '%-36s %10d bytes (other %10d)  differing lines: %d\n' "$n" "$(stat -c %s "$f")" "$(stat -c %s "$OUT/other/$n")" "$d"
    [ "$d" = 0 ] || rc=1
done
if diff "$OUT/other/resources.txt" "$OUT/this/resources.txt" > "$OUT/resources.diff"; then
    echo "resource lines equal:"; cat "$OUT/this/resources.txt"
else
    echo "resource lines DIFFER:"; cat "$OUT/resources.diff"; rc=1
fi
[ $rc = 0 ] && echo "SAME" || echo "DIFFERENT"
exit $rc

#!/bin/bash
# Whole-file identity of the device code of two trees: compiles each named source of both trees to gfx950 assembly with the flags build.py gives it (each side from its
# own root, by the same relative path, so that no path enters the text), drops comment-only lines and the .file / .ident directives, and diffs.
#   tools/asm_identity.sh <parent tree> <result tree> <out dir> [source.hip ...]      (default: the register-weight kernels and the two 1x1 kernels)
# Prints one markdown table row per source (sha256 of both stripped texts) and exits 1 when any pair differs; the stripped texts stay in <out dir>/{a,b}/.
set -e -o pipefail
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); mkdir -p "$3"; OUT=$(cd "$3" && pwd); shift 3
SRCS=${*:-conv3x3_rw.hip conv3x3_ps4.hip conv3x3_ps9.hip arsb32c.hip conv64_q8.hip conv64_sq.hip arsb_sq.hip conv64_s.hip conv1x1.hip conv1x1_f2.hip}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$OUT/a" "$OUT/b"
one() {      # <tree> <side> <source>
    local stem=${3%.hip} extra
    extra=$(cd "$1" && python -c "from moephoto_amd import build; print(' '.join(build.EXTRA_FLAGS.get('$3', [])))")
    (cd "$1" && $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip --cuda-device-only -S -cuid=moe_$stem $extra moephoto_amd/csrc/$3 -o "$OUT/$2/$stem.raw.s")
    grep -v -E '^[[:space:]]*(;|//|\.file|\.ident)' "$OUT/$2/$stem.raw.s" > "$OUT/$2/$stem.s"
    rm "$OUT/$2/$stem.raw.s"
}
for s in $SRCS; do
    one "$A" a $s &
    one "$B" b $s &
    while [ $(jobs -r | wc -l) -ge 8 ]; do wait -n; done
done
wait
bad=0
echo "| source | parent sha256 | result sha256 | diff |"
echo "|---|---|---|---|"
for s in $SRCS; do
    stem=${s%.hip}
    ha=$(sha256sum < "$OUT/a/$stem.s" | cut -d' ' -f1); hb=$(sha256sum < "$OUT/b/$stem.s" | cut -d' ' -f1)
    if cmp -s "$OUT/a/$stem.s" "$OUT/b/$stem.s"; then d=empty; else d=DIFFERS; bad=1; fi
    echo "| $s | $ha | $hb | $d |"
done
exit $bad

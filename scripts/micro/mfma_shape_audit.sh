#!/bin/bash
# Static audit of the MFMA-shape micro-benchmark (scripts/micro/mfma_shape.hip), no GPU needed: compiles it to ISA and lists what
# each kernel's TIMED loop holds - the basic block around the MFMA_SHAPE_BODY markers up to its backward branch.  The comparison of
# the two instruction shapes is valid only while that block is matrix instructions and scalar loop control (plus, in the *_lds
# kernels, the ds_read_b128 operand reads and their s_waitcnt): any v_accvgpr_* or other vector ALU instruction makes the loop
# measure VALU issue instead (as scripts/micro/mfma_peak16.hip did: 96 v_accvgpr moves per 32 MFMAs).  Over the whole kernel it counts
# compiler references to the accumulation registers the asm owns (must be 0).  Exit status 1 on a violation or a failed compile.
# HIPCC / ARCH: the compiler and target the library itself was built with (csrc/Makefile honours the same variables).
set -e
cd "$(dirname "$0")"
OUT=${MFMA_SHAPE_AUDIT_DIR:-/tmp/mfma_shape_audit}; mkdir -p $OUT
rm -f $OUT/mfma_shape.s $OUT/mfma*_*.s $OUT/*.range   # never audit what an earlier run left behind
if ! ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=${ARCH:-gfx950} -O3 -S --cuda-device-only "$@" mfma_shape.hip -o $OUT/mfma_shape.s 2> $OUT/hipcc.log; then
  grep -E "error" $OUT/hipcc.log || cat $OUT/hipcc.log
  echo "AUDIT FAILED: mfma_shape.hip does not compile"; exit 1
fi
BAD=0
for K in mfma32_reg mfma16_reg mfma32_lds mfma16_lds; do
  awk "/^$K:/,/^.Lfunc_end/" $OUT/mfma_shape.s > $OUT/$K.s
  # the loop: from the last label in front of the BEGIN marker to the first branch behind the END marker
  awk '/^\.LBB[0-9_]+:/{lab=NR} /MFMA_SHAPE_BODY_BEGIN/{b=lab} /MFMA_SHAPE_BODY_END/{e=1} e && /s_cbranch/{print b, NR; exit}' $OUT/$K.s > $OUT/$K.range
  read B E < $OUT/$K.range
  LINE=$(awk -v B=${B:-0} -v E=${E:-0} 'NR>=B && NR<=E {
      sub(/;.*/, ""); if ($0 ~ /^[ \t]*$/ || $0 ~ /^[.A-Za-z_0-9]+:/ || $1 ~ /^\./) next
      if ($1 ~ /^v_mfma_f32_(32x32x16|16x16x32)_bf16$/) m++
      else if ($1 ~ /^v_accvgpr/) av++
      else if ($1 ~ /^v_/) valu++
      else if ($1 == "ds_read_b128") ds++
      else if ($1 ~ /^s_waitcnt/) w++
      else if ($1 ~ /^s_/) sc++
      else other++ }
    END { printf "mfma %d ds_read_b128 %d s_waitcnt %d scalar %d v_accvgpr %d other_valu %d other %d", m, ds, w, sc, av, valu, other }' $OUT/$K.s)
  # whole kernel: instructions outside the asm statements that name an accumulation register (a compiler value in a register the asm owns)
  REFS=$(awk '/ASMSTART/{a=1} /ASMEND/{a=0} { if(!a && ($0 ~ /[ ,\[]a[0-9]+[ ,\]:]|[ ,]a\[[0-9]/) && $0 !~ /^[ \t]*;/ && $0 !~ /\.amdhsa|\.sgpr|\.vgpr|\.agpr/) n++ } END{print n+0}' $OUT/$K.s)
  LINE="$LINE compiler_acc_refs $REFS"
  echo "AUDIT $K: loop lines ${B:-?}-${E:-?} $LINE"
  case $K in
    mfma32_reg) WANT="mfma 16 ds_read_b128 0 s_waitcnt 0 " ;;
    mfma16_reg) WANT="mfma 32 ds_read_b128 0 s_waitcnt 0 " ;;
    mfma32_lds) WANT="mfma 16 ds_read_b128 16 s_waitcnt 2 " ;;
    mfma16_lds) WANT="mfma 32 ds_read_b128 16 s_waitcnt 2 " ;;
  esac
  case "$LINE" in
    "$WANT"*" v_accvgpr 0 other_valu 0 other 0 compiler_acc_refs 0") ;;
    *) echo "  VIOLATION in $K: want '$WANT... v_accvgpr 0 other_valu 0 other 0 compiler_acc_refs 0'"; BAD=1 ;;
  esac
done
exit $BAD

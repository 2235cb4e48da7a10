#!/bin/bash
# build_variant.sh <name> [hipcc -D flags...]: a build variant of the kernels
# (the units split from rnt_kernels.hip -- rnt_col, rnt_rows, rnt_kernels -- and
# rnt_plane.hip, or with PLANE_ONLY=1 only rnt_plane.hip,
# with the given flags) linked with the normal objects of the rest ->
# toy-heaan-ckks_amd/lib/variants/librnsntt_<name>.so (for same-box A/B runs:
# tools/ab.sh).  KSRC=<file> compiles another version of the unit of the same
# base name (KSRC=/tmp/x/rnt_rows.hip in place of csrc/rnt_rows.hip).
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/toy-heaan-ckks_amd/csrc; L=$ROOT/toy-heaan-ckks_amd/lib; V=$L/variants
mkdir -p $V
HF="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$C"
KUNITS="rnt_col rnt_rows rnt_kernels"
KOBJS=""; for u in $KUNITS; do KOBJS="$KOBJS $L/$u.o"; done
OBJS_REST="$L/rnt_encode.o $L/rnt_sample.o $L/rnt_raise.o $L/rnt_api.o"
# the source of unit $1: KSRC where its base name is the unit's
src_of() { if [ "$(basename "${KSRC:-}" .hip)" = "$1" ]; then echo "$KSRC"; else echo "$C/$1.hip"; fi; }
if [ "${MF_ONLY:-0}" = "1" ]; then
  # only rnt_mfma.hip with the flags (KSRC=<file>: another version of it), the rest as built
  /opt/rocm/bin/hipcc $HF "$@" -c ${KSRC:-$C/rnt_mfma.hip} -o $V/m_$NAME.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $KOBJS $L/rnt_plane.o $V/m_$NAME.o $OBJS_REST -o $V/librnsntt_$NAME.so
  echo $V/librnsntt_$NAME.so
  exit 0
fi
if [ "${PLANE_ONLY:-0}" = "1" ]; then
  # KSRC=<file> compiles another version of rnt_plane.hip
  /opt/rocm/bin/hipcc $HF "$@" -c ${KSRC:-$C/rnt_plane.hip} -o $V/p_$NAME.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $KOBJS $V/p_$NAME.o $L/rnt_mfma.o $OBJS_REST -o $V/librnsntt_$NAME.so
else
  if [ -n "${KSRC:-}" ] && ! echo " $KUNITS rnt_plane " | grep -q " $(basename "$KSRC" .hip) "; then
    echo "KSRC=$KSRC: its base name is none of: $KUNITS rnt_plane" >&2
    exit 2
  fi
  VOBJS=""
  for u in $KUNITS rnt_plane; do
    rm -f $V/${u#rnt_}_$NAME.o  # (the units compile side by side: a failed one leaves no object)
    /opt/rocm/bin/hipcc $HF "$@" -c "$(src_of $u)" -o $V/${u#rnt_}_$NAME.o &
    VOBJS="$VOBJS $V/${u#rnt_}_$NAME.o"
  done
  wait
  for o in $VOBJS; do test -f $o; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $VOBJS $L/rnt_mfma.o $OBJS_REST -o $V/librnsntt_$NAME.so
fi
echo $V/librnsntt_$NAME.so

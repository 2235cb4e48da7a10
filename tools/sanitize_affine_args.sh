#!/usr/bin/env bash
# ASan + UBSan run of the argument rules of rnt_ct_mul_relin_rescale_affine_hybrid
# from a stand-alone program (tests/cpp/affine_args_check.cpp, its own main): the
# host code of rnt_api.cpp is compiled with the sanitizers (each -fsanitize=
# after -Xarch_host: device code is not instrumented), linked with the library's
# other objects as `make` built them and with the program, and the program is
# run as it is -- nothing is preloaded and no GPU is needed (every call it makes
# is refused before any device work).
#
# Usage: tools/sanitize_affine_args.sh [log]   (default log: profiles/affine_args_sanitizer.log)
set -euo pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/affine_args_sanitizer.log}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=build/asan
LIB=toy-heaan-ckks_amd/lib
CS=toy-heaan-ckks_amd/csrc
mkdir -p "$OUT"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
for o in rnt_col rnt_rows rnt_kernels rnt_plane rnt_mfma rnt_encode rnt_sample rnt_raise; do
  test -f $LIB/$o.o || { echo "$LIB/$o.o is missing: run make first" >&2; exit 2; }
done
{
  echo "# tools/sanitize_affine_args.sh"
  echo "# rnt_api.cpp and tests/cpp/affine_args_check.cpp: $HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 $SAN"
} > "$LOG"
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $SAN -c $CS/rnt_api.cpp -o $OUT/rnt_api_host.o
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $SAN -I include -I $CS -c tests/cpp/affine_args_check.cpp \
  -o $OUT/affine_args_check.o
$HIPCC --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
  $OUT/affine_args_check.o $OUT/rnt_api_host.o $LIB/rnt_col.o $LIB/rnt_rows.o $LIB/rnt_kernels.o $LIB/rnt_plane.o $LIB/rnt_mfma.o $LIB/rnt_encode.o \
  $LIB/rnt_sample.o $LIB/rnt_raise.o -o $OUT/affine_args_check
set +e
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
  $OUT/affine_args_check >> "$LOG" 2>&1
rc=$?
set -e
reports=$(grep -c "ERROR: AddressSanitizer\|runtime error:" "$LOG" || true)
echo "# sanitizer reports: $reports" >> "$LOG"
echo "# exit status $rc" >> "$LOG"
tail -4 "$LOG"
exit $rc

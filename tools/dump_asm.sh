#!/bin/bash
# Device assembly of the product translation units (gfx950), one .s per unit: tools/dump_asm.sh <outdir> [unit ...]
# Used to check that a source clean-up leaves the generated code untouched (diff of two dumps) and to read wait counts.
# A unit is NAME (os2d_amd/csrc/NAME.hip -> NAME.s) or csrc_train/NAME (os2d_amd/csrc_train/NAME.hip -> train_NAME.s, with the
# flags build.py gives the units of libos2d_train.so); without units: all of both directories.
OUT=$1; shift
ROOT=$(dirname "$0")/../os2d_amd
mkdir -p "$OUT"
UNITS=${@:-$(cd $ROOT/csrc && ls *.hip | sed 's/\.hip$//') $(cd $ROOT && ls csrc_train/*.hip | sed 's/\.hip$//')}
for u in $UNITS; do
  case $u in
    csrc_train/objective) src=$ROOT/$u.hip; out=train_objective; extra=-ffp-contract=off ;;   # build.py: TRAIN.unit_flags
    csrc_train/*) src=$ROOT/$u.hip; out=train_${u#csrc_train/}; extra= ;;
    *) src=$ROOT/csrc/$u.hip; out=$u; extra= ;;
  esac
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc -Xclang -target-feature -Xclang -packed-fp32-ops $OS2D_EXTRA_HIPCC_FLAGS $extra \
        -S --offload-device-only -o "$OUT/$out.s" "$src" 2>/dev/null &
done
wait

#!/bin/bash
# builds the instrumented variant of the library (-DE2E_FAST_PROFILE -DE2E_BEAM_PROFILE) as build/diag/prof_lib.so (or
# build/diag/$PROF_OUT); E2E_EXTRA_DEFS adds -D options (a switch of an experiment's branch);
# PROF_FILES limits the sources compiled with the options to the listed ones (the others come from the regular build).
# The beam kernels' sources give one object per input dtype, as in the Makefile; E2E_BEAM_PROFILE goes to the f32 object of
# ctc_beam_lds.hip alone: the counters and their readers live in the object whose kernels write them.
set -e
cd "$(dirname "$0")/../../end2end_amd/csrc"; mkdir -p ../../build/diag
out=${PROF_OUT:-prof_lib.so}; tmp=/tmp/e2e_prof_${out%.so}; mkdir -p $tmp
objs=
for f in *.hip; do
  variants=-; [[ $f == ctc_beam_lds.hip || $f == ctc_beam_general.hip ]] && variants="f32:float f64:double f16:e2e::f16_t bf16:e2e::bf16_t"
  for v in $variants; do
    o=${f%.hip}.o; extra=
    [[ $v != - ]] && { o=${f%.hip}.${v%%:*}.o; extra=-DE2E_BEAM_IO=${v#*:}; }
    [[ $f == ctc_loss_fast*.hip ]] && extra=-fno-slp-vectorize
    [[ $o == ctc_beam_lds.f32.o ]] && extra="$extra -DE2E_BEAM_PROFILE"
    if [ -z "$PROF_FILES" ] || [[ " $PROF_FILES " == *" $f "* ]]; then
      /opt/rocm/bin/hipcc $extra -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DE2E_FAST_PROFILE $E2E_EXTRA_DEFS -ffp-contract=off -c $f -o $tmp/$o &
      objs="$objs $tmp/$o"
    else objs="$objs $o"; fi
  done
done; wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build/diag/$out $objs -lz

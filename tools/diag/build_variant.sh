#!/bin/bash
# A variant of the library for same-process A/B timing (tools/diag/ab_time.py):
#   tools/diag/build_variant.sh NAME "-DFOO -DBAR" [file.hip ...]
# recompiles the listed sources (default: ctc_loss_fast.hip) with the extra options, links them with the objects of the
# regular build (run `make -C end2end_amd/csrc` first) and leaves build/diag/ab_NAME.so (build/ is git-ignored, but
# travels to the GPU box).  The beam kernels' sources give one object per input dtype, as in the Makefile.
set -e
cd "$(dirname "$0")/../../end2end_amd/csrc"; mkdir -p ../../build/diag /tmp/e2e_var_$1
name=$1; defs=$2; shift; shift || true
files=${@:-ctc_loss_fast.hip}
objs=
for f in *.hip; do
  variants=-; [[ $f == ctc_beam_lds.hip || $f == ctc_beam_general.hip ]] && variants="f32:float f64:double f16:e2e::f16_t bf16:e2e::bf16_t"
  for v in $variants; do
    o=${f%.hip}.o; extra=
    [[ $v != - ]] && { o=${f%.hip}.${v%%:*}.o; extra=-DE2E_BEAM_IO=${v#*:}; }
    [[ $f == ctc_beam_general.hip ]] && extra="$extra -DE2E_BEAM_CUT=false"
    [[ $f == ctc_loss_fast*.hip ]] && extra=-fno-slp-vectorize
    if [[ " $files " == *" $f "* ]]; then
      /opt/rocm/bin/hipcc $extra -O3 -std=c++17 -fPIC --offload-arch=gfx950 $defs -ffp-contract=off -c $f -o /tmp/e2e_var_$name/$o &
      objs="$objs /tmp/e2e_var_$name/$o"
    else objs="$objs $o"; fi
  done
done
# the general kernel's pruned instances: objects of their own from the same source (-DE2E_BEAM_CUT=true)
for v in f32:float f64:double f16:e2e::f16_t bf16:e2e::bf16_t; do
  o=ctc_beam_general_cut.${v%%:*}.o
  if [[ " $files " == *" ctc_beam_general.hip "* ]]; then
    /opt/rocm/bin/hipcc -DE2E_BEAM_IO=${v#*:} -DE2E_BEAM_CUT=true -O3 -std=c++17 -fPIC --offload-arch=gfx950 $defs -ffp-contract=off -c ctc_beam_general.hip -o /tmp/e2e_var_$name/$o &
    objs="$objs /tmp/e2e_var_$name/$o"
  else objs="$objs $o"; fi
done; wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build/diag/ab_$name.so $objs -lz

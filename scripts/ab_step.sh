#!/bin/bash
# Interleaved step-level A/B on ONE box:
#   scripts/ab_step.sh ROUNDS label[:lib=PATH][:dir=PATH][:set=name=v,...][:env=NAME=V][:arg=--model=NAME] ...
# prints ms_per_step of `bench.py --no-cpu-baseline --no-kernel-events` per label and round.  dir=PATH runs the bench.py of
# another checkout (e.g. an export of the parent commit with its own built library) instead of this tree's.  The first run
# that fails ends the script: nothing more is started on a GPU that may have faulted.
root=$(cd "$(dirname "$0")/.." && pwd)
rounds=$1; shift
for i in $(seq 1 $rounds); do
  for spec in "$@"; do
    label=${spec%%:*}; lib=""; set=""; dir=""; args=""
    IFS=':' read -ra parts <<< "$spec"
    envs=""
    for p in "${parts[@]:1}"; do case $p in lib=*) lib=${p#lib=};; dir=*) dir=${p#dir=};; set=*) set=${p#set=};; env=*) envs="$envs ${p#env=}";; arg=*) args="$args ${p#arg=}";; esac; done
    if [ -n "$lib" ]; then export PAI_HIP_LIB=$root/$lib; else unset PAI_HIP_LIB; fi
    cd "$root/$dir" || exit 1
    out=$(env $envs timeout -k 10 200 python bench.py --no-cpu-baseline --no-kernel-events $args ${set:+--set $set} 2>/dev/null)
    rc=$?
    if [ $rc -ne 0 ]; then echo "$label failed (exit $rc)"; exit $rc; fi
    ms=$(echo "$out" | python3 -c "import sys,json; print(json.loads(sys.stdin.read().strip().splitlines()[-1])['ms_per_step'])") || exit 1
    echo "$label $ms"
  done
done

#!/bin/bash
# same-box A/B of two builds of the library (_ab/old.so, _ab/new.so: each run loads its build through S2E_LIB_PATH, the in-tree one is never touched; ABAB):  bash tools/ab_so.sh ["<kernel regex>"]
for r in 1 2; do
for v in old new; do
S2E_LIB_PATH=_ab/$v.so python bench.py --steps 50 --warmup 10 --no-cpu-baseline --no-extras --no-kernel-events 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', round(d['value'],1), round(d['ms_per_step'],3))"
done; done
if [ -n "$1" ]; then for v in old new; do S2E_LIB_PATH=_ab/$v.so bash tools/kt_kernels.sh "$1" AB=$v; done; fi
